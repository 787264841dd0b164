"""rrx_multi_contains_corpus on a box without a device: the header declares it, the library exports it, and it refuses null
arguments before any device call."""
import ctypes as C
import os
import re

import roaringregex_amd as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 2


def test_the_header_declares_it_and_the_library_exports_it():
    hdr = open(os.path.join(ROOT, "include", "rrx.h")).read()
    assert re.search(r"^int rrx_multi_contains_corpus\(const rrx_multi \*m, const rrx_corpus \*c, uint32_t \*d_mask, void \*stream\);$", hdr, re.M)
    lib = C.CDLL(os.path.join(ROOT, "roaringregex_amd", "librrx.so"))
    assert hasattr(lib, "rrx_multi_contains_corpus")
    assert "rrx_multi_contains_corpus" in rr.ABI_SYMBOLS and hasattr(rr.RMulti, "contains_corpus")


def test_null_arguments_are_refused_before_any_device_call():
    """(This box may have no device at all.  The entry looks at no argument before it has seen that all three are there: a buffer
    of zeros stands for the handles that cannot be made here.)"""
    m = rr.RMulti(["a", "b"])
    buf = (C.c_uint64 * 64)()
    p = C.cast(buf, C.c_void_p)
    f = rr._L.rrx_multi_contains_corpus
    assert f(None, p, p, None) == ERR_ARG and b"null argument" in rr._L.rrx_last_error()
    assert f(m._h, None, p, None) == ERR_ARG
    assert f(m._h, p, None, None) == ERR_ARG
    assert f(None, None, None, None) == ERR_ARG
