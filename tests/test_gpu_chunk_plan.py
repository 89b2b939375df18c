"""The pool-chunk plan the contexts hand their sweeps (csrc/fic_sweep_chunks.h behind fic_capi.cpp, fic_capi_rgb.cpp and
fic_capi_rgb_lsq.cpp), end to end on small shapes: what a context reports after an encode -- info()["chunks"] of a grey context,
the kernel name of a colour context's matrix-core search, last_lsq_chunks() of its least-squares search -- equals
tests/golden/ctx_chunks.json, recorded from commit 4699b90 (the last one whose C ABI carried the rules itself) with record(),
and every codebook equals the "chunks" = 1 codebook of the same context bit for bit.  The CPU table tests/golden/sweep_chunks.txt
checks the rules; this checks the workgroup counts and residencies the callers hand them."""
import json
import os

import numpy as np
import pytest

import fic_amd
from fic_amd import capi
from oracle import fic_oracle as fo

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TABLE = os.path.join(GOLDEN, "ctx_chunks.json")

GEOMS = [(64, 4), (128, 8)]                     # (side, B): full search
CHUNKS = (0, 3, 7)
GREY = [(w, B, n_iso, planes) for w, B in GEOMS for n_iso in (1, 8) for planes in (1, 3)]
RGB = [(w, B, n_iso) for w, B in GEOMS for n_iso in (1, 8)]


def _grey_image(w, planes):
    g = np.load(os.path.join(GOLDEN, "lena_grey_256.npy"))
    return np.stack([np.ascontiguousarray(g[16 * p:16 * p + w, 32 * p:32 * p + w]) for p in range(planes)])


def _rgb_image(w):
    rgb = np.load(os.path.join(GOLDEN, "lena_colored_256.npy"))
    return fo.rgb_to_argb(np.ascontiguousarray(rgb[96:96 + w, 64:64 + w]))


def _same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in a)


def grey_case(w, B, n_iso, planes):
    """{"<mode>/<chunks>": info()["chunks"]} over every sweep the geometry allows, and whether every codebook equalled the
    one-chunk codebook of its mode."""
    out, same = {}, True
    with fic_amd.Encoder(w, w, B, None, n_iso, planes) as enc:
        enc.set_gray(_grey_image(w, planes))
        modes = [("sweep2", 0, 2), ("sweep6", 0, 6), ("lsq", 1, 0)]
        if B == 8 and n_iso == 8 and enc.info()["NR"] == 1:
            modes.append(("sweep5", 0, 5))
        if capi.has_xcheck():
            modes.append(("sweep3", 0, 3))
        for name, search, sweep in modes:
            enc.set_option("sweep", 0)
            enc.set_option("search", search)
            enc.set_option("sweep", sweep)
            enc.set_option("lsq_engine", 0)
            enc.set_option("chunks", 1)
            enc.encode()
            one = enc.results()
            assert enc.info()["chunks"] == 1
            for ch in CHUNKS:
                enc.set_option("chunks", ch)
                enc.encode()
                out[f"{name}/{ch}"] = enc.info()["chunks"]
                same = same and _same(enc.results(), one)
    return out, same


def rgb_case(w, B, n_iso):
    """{"sweep2/<chunks>": kernel name, "lsq/<chunks>": last_lsq_chunks()} and whether every codebook equalled the one-chunk one."""
    out, same = {}, True
    Dw = capi.geometry(w, w, B)[2]
    with capi.RgbEncoder(w, w, B, Dw, n_iso=n_iso) as enc:
        enc.set_argb(_rgb_image(w))
        for name, search, sweep in (("sweep2", 0, 2), ("lsq", 1, 0)):
            enc.set_option("search", search)
            enc.set_option("sweep", sweep)
            enc.set_option("lsq_engine", 0)
            enc.set_option("chunks", 1)
            enc.encode()
            one = enc.results()
            for ch in CHUNKS:
                enc.set_option("chunks", ch)
                enc.encode()
                out[f"{name}/{ch}"] = enc.last_kernel() if search == 0 else enc.last_lsq_chunks()
                same = same and _same(enc.results(), one)
    return out, same


def grey_id(w, B, n_iso, planes):
    return f"grey-{w}x{w}-B{B}-iso{n_iso}-p{planes}"


def rgb_id(w, B, n_iso):
    return f"rgb-{w}x{w}-B{B}-iso{n_iso}"


def record():
    """What this build reports for every case: the content of ctx_chunks.json when run on the commit named above."""
    table = {grey_id(*c): grey_case(*c)[0] for c in GREY}
    table.update({rgb_id(*c): rgb_case(*c)[0] for c in RGB})
    return table


@pytest.fixture(scope="module")
def table():
    with open(TABLE) as f:
        return json.load(f)


def _compare(got, want, with_xcheck):
    want = {k: v for k, v in want.items() if with_xcheck or not k.startswith("sweep3/")}
    print(got)
    assert got == want


@pytest.mark.parametrize("w,B,n_iso,planes", GREY, ids=[grey_id(*c) for c in GREY])
def test_grey_chunks_as_recorded(table, w, B, n_iso, planes):
    got, same = grey_case(w, B, n_iso, planes)
    want = table[grey_id(w, B, n_iso, planes)]
    assert any(k.startswith("sweep3/") for k in want), "the table was recorded from a build with the cross-check sweeps"
    _compare(got, want, capi.has_xcheck())
    assert same, "a codebook depends on the chunk count"


@pytest.mark.parametrize("w,B,n_iso", RGB, ids=[rgb_id(*c) for c in RGB])
def test_rgb_chunks_as_recorded(table, w, B, n_iso):
    got, same = rgb_case(w, B, n_iso)
    _compare(got, table[rgb_id(w, B, n_iso)], True)
    assert same, "a codebook depends on the chunk count"
