"""Records what the three *_set_option entries answer for the option names the handles share (tests/golden/option_texts.json,
replayed by tests/test_gpu_option_texts.py): for every name one step below and above its range, the values of a gap inside it,
both boundaries, then an unknown and a NULL name -- return code and, for a refusal, fic_last_error()'s text.  Nothing is encoded;
the contexts are 32 x 32, B = 4, one plane (quadtree: 8 -> 4).  Run it on the library whose texts are to be pinned:

    python tools/record_option_texts.py tests/golden/option_texts.json
"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fic_amd  # noqa: E402

INT_MAX = 2 ** 31 - 1
# name: the values tried, in this order (the last accepted one stays in force; none changes what a later case answers)
VALUES = {
    "search": (-1, 2, 1, 0),
    "chunks": (-1, INT_MAX, 0),
    "q_eshift": (-13, 5, -12, 4, 0),
    "lsq_tau_widen": (-1, 1, 7, 25, 8, 24, 0),
    "lsq_engine": (-1, 2, 1, 0),
    "lsq_q_eshift": (-13, 5, -12, 4, 0),
    "time_sweep": (-1, 2, 1, 0),
    "sweep_stats": (-1, 2, 1, 0),
    "no_such_option": (0,),
    None: (0,),
}
HANDLES = {
    "grey": ("fic_ctx", lambda L: L.fic_ctx_create(0, 32, 32, 4, 8, 1, 1)),
    "rgb": ("fic_rgb_ctx", lambda L: L.fic_rgb_ctx_create_iso(0, 32, 32, 4, 8, 1, 1)),
    "qt": ("fic_qt_ctx", lambda L: L.fic_qt_ctx_create(0, 0, 32, 32, 8, 4, 0, 1, 1)),
}


def replay(handle, cases):
    """[(code, message)] of `cases` [(name, value)] on a fresh context of kind `handle`; message is "" for an accepted value."""
    L = fic_amd.capi.lib()
    prefix, create = HANDLES[handle]
    for fn, res in ((prefix + "_create", C.c_void_p), ("fic_rgb_ctx_create_iso", C.c_void_p)):
        getattr(L, fn).restype = res
    h = C.c_void_p(create(L))
    if not h:
        raise RuntimeError(fic_amd.capi.last_error())
    set_option = getattr(L, prefix + "_set_option")
    set_option.restype, set_option.argtypes = C.c_int, [C.c_void_p, C.c_char_p, C.c_int]
    destroy = getattr(L, prefix + "_destroy")
    destroy.restype, destroy.argtypes = None, [C.c_void_p]
    try:
        out = []
        for name, value in cases:
            rc = set_option(h, None if name is None else name.encode(), value)
            out.append((rc, fic_amd.capi.last_error() if rc else ""))
        return out
    finally:
        destroy(h)


def main(path):
    rows = []
    for handle in HANDLES:
        cases = [(name, v) for name, vals in VALUES.items() for v in vals]
        for (name, value), (code, message) in zip(cases, replay(handle, cases)):
            rows.append({"handle": handle, "name": name, "value": value, "code": code, "message": message})
    with open(path, "w") as f:
        json.dump({"library": fic_amd.capi.lib().fic_version().decode(), "cases": rows}, f, indent=1)
        f.write("\n")
    print(f"{len(rows)} cases -> {path}")


if __name__ == "__main__":
    main(sys.argv[1])
