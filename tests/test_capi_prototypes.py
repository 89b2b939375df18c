"""The ctypes prototypes come from include/fic.h (capi.prototypes): every declared entry is typed after lib(), the types that
are easy to get wrong are the header's, and a type the parser does not know is an error."""
import ctypes as C

import pytest

from fic_amd import capi


def test_every_declared_symbol_is_typed():
    L = capi.lib()
    names = capi.declared_symbols()
    assert len(names) == len(capi.prototypes()) >= 121
    for name in names:
        assert getattr(L, name).argtypes is not None, name


def test_the_types_the_callers_rely_on():
    L = capi.lib()
    assert L.fic_write_run_gray.restype is C.c_int64
    assert L.fic_ctx_create.restype is C.c_void_p and L.fic_rgb_ctx_create_iso.restype is C.c_void_p and L.fic_qt_ctx_create.restype is C.c_void_p
    assert L.fic_debug_live_memory.argtypes == [C.POINTER(C.c_int64)]            # int64_t out4[4]: an array parameter is a pointer
    assert L.fic_qt_ctx_encode_rd.argtypes == [C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.c_void_p]
    assert L.fic_release_cache.restype is None and L.fic_release_cache.argtypes == []
    assert L.fic_version.restype is C.c_char_p
    assert L.fic_ctx_result_device_ptrs.argtypes == [C.c_void_p] + [C.POINTER(C.c_void_p)] * 7
    assert L.fic_ctx_set_option.argtypes == [C.c_void_p, C.c_char_p, C.c_int]
    assert L.fic_decode_rgb_run.argtypes[1] is C.c_int64 and L.fic_decode_rgb_run.argtypes[3] == C.POINTER(C.c_int32)


@pytest.mark.parametrize("decl", ["size_t n", "unsigned flags", "struct foo* p", "int** pp", "fic_ctx ctx", "long long v", ""])
def test_an_unknown_type_is_an_error(decl):
    with pytest.raises(capi.FicError):
        capi._ctype(decl, "a test")


def test_handle_classes_share_the_base():
    import fic_amd
    assert fic_amd.RgbEncoder is capi.RgbEncoder
    for cls in (fic_amd.Encoder, fic_amd.RgbEncoder, fic_amd.QuadtreeEncoder):
        assert issubclass(cls, capi.Handle)
        for m in ("close", "__del__", "__enter__", "__exit__", "sync", "sweep_time", "last_kernel", "set_option", "lsq_error"):
            assert m not in vars(cls), (cls.__name__, m)
