"""The lease of the one-shot entries on the cached single-image contexts (ficd::Lease, csrc/fic_internal.h): a context that ran
a least-squares quadtree level goes back in the reference's mode -- the reference one-shot on the same geometry, which takes that
very context from the cache, returns the reference codebook -- and a refused one-shot parks nothing.  64 x 64, B = 8, n_iso = 1.
(The fixed-B twins: test_cached_contexts_stay_in_reference_mode of tests/test_gpu_lsq.py and tests/test_gpu_rgb_lsq.py.)"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import same_f32  # noqa: E402

import fic_amd  # noqa: E402
from fic_amd import capi  # noqa: E402
from oracle import fic_oracle as fo  # noqa: E402

pytestmark = pytest.mark.gpu

W = H = 64
B = 8
ZERO = dict.fromkeys(capi.LIVE_MEMORY_FIELDS, 0)


def _same_codebook(got, want, floats):
    for k in ("idx_local", "iso", "qrows"):
        assert (got[k] == want[k]).all(), k
    for k in floats:
        assert same_f32(got[k], want[k]), k


def test_grey_quadtree_levels_go_back_in_reference_mode(lena64):
    capi.release_cache()
    wK = fo.geometry(W, H, B)[2]                              # the quadtree's wK = 0 is full search: the one-shot's context of B = 8
    ref = capi.encode_gray_oneshot(lena64, B, wK, 1)
    tree = capi.encode_gray_quadtree(lena64, B, 4, 0, 1, 200.0)
    lsq = capi.encode_gray_quadtree(lena64, B, 4, 0, 1, 200.0, search="lsq")
    assert lsq.shape[1] == tree.shape[1] and not (lsq.shape == tree.shape and (lsq == tree).all())
    _same_codebook(capi.encode_gray_oneshot(lena64, B, wK, 1), ref, ("a", "b"))
    again = capi.encode_gray_quadtree(lena64, B, 4, 0, 1, 200.0)
    assert again.shape == tree.shape and (again == tree).all()
    capi.release_cache()
    assert capi.live_memory() == ZERO


def test_colour_quadtree_levels_go_back_in_reference_mode(lena_colored):
    capi.release_cache()
    argb = fo.rgb_to_argb(np.ascontiguousarray(lena_colored[96:160, 64:128]))
    wK = fo.geometry(W, H, B)[2]
    ref = fic_amd.encode_rgb(argb, W, H, B, wK)
    tree = capi.encode_rgb_quadtree_iso(argb, W, H, B, 4, 0, 1, 3000.0)
    lsq = capi.encode_rgb_quadtree_iso(argb, W, H, B, 4, 0, 1, 3000.0, search="lsq")
    assert lsq.shape[1] == tree.shape[1] and not (lsq.shape == tree.shape and (lsq == tree).all())
    _same_codebook(fic_amd.encode_rgb(argb, W, H, B, wK), ref, ("a", "bR", "bG", "bB"))
    again = capi.encode_rgb_quadtree_iso(argb, W, H, B, 4, 0, 1, 3000.0)
    assert again.shape == tree.shape and (again == tree).all()
    capi.release_cache()
    assert capi.live_memory() == ZERO


def test_a_refused_one_shot_parks_nothing(lena64, lena_colored):
    capi.release_cache()
    before = capi.live_memory()
    assert before == ZERO
    L = capi.lib()
    g = np.ascontiguousarray(lena64)
    nr = (W // B) * (H // B)
    a, b = np.zeros(nr, np.float32), np.zeros(nr, np.float32)
    for fn, tail in ((L.fic_encode_gray_u8, ()), (L.fic_encode_gray_lsq_u8, (None,))):      # grey: a NULL results pointer
        rc = fn(capi.ptr(g, C.c_uint8), W, H, B, 4, 1, 0, None, capi.ptr(a, C.c_float), capi.ptr(b, C.c_float), None, None, *tail)
        assert rc == -3 and "null argument" in capi.last_error()
        assert capi.live_memory() == before
    argb = fo.rgb_to_argb(np.ascontiguousarray(lena_colored[:H, :W]))
    for search in ("reference", "lsq"):                                                      # colour: n_iso = 3
        with pytest.raises(fic_amd.FicError) as e:
            fic_amd.encode_rgb(argb, W, H, B, 4, n_iso=3, search=search)
        assert e.value.code == -3 and "n_iso=3" in str(e.value)
        assert capi.live_memory() == before
