"""rrx_search_longest_corpus on a box without a device: the header declares it, the library exports it, the Python and C++ layers
reach it, and it refuses null arguments before any device call."""
import ctypes as C
import os
import re

import roaringregex_amd as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 2


def test_the_header_declares_it_and_the_library_exports_it():
    hdr = open(os.path.join(ROOT, "include", "rrx.h")).read()
    assert re.search(r"^int rrx_search_longest_corpus\(const rrx_regex \*re, const rrx_corpus \*c, uint32_t \*d_start, uint32_t \*d_end, void \*stream\);$",
                     hdr, re.M)
    lib = C.CDLL(os.path.join(ROOT, "roaringregex_amd", "librrx.so"))
    assert hasattr(lib, "rrx_search_longest_corpus")
    assert "rrx_search_longest_corpus" in rr.ABI_SYMBOLS and hasattr(rr.RRegex, "search_longest_corpus")
    facade = open(os.path.join(ROOT, "include", "rregex.hpp")).read()
    assert re.search(r"void search_longest_corpus\(const rrx_corpus \*corpus, uint32_t \*d_start, uint32_t \*d_end, void \*stream = nullptr\)", facade)


def test_null_arguments_are_refused_before_any_device_call():
    """(This box may have no device at all.  The entry looks at no argument before it has seen that all four are there: a buffer of
    zeros stands for the corpus that cannot be made here.)"""
    r = rr.RRegex("ab+c")
    buf = (C.c_uint64 * 64)()
    p = C.cast(buf, C.c_void_p)
    f = rr._L.rrx_search_longest_corpus
    assert f(None, p, p, p, None) == ERR_ARG and b"null argument" in rr._L.rrx_last_error()
    assert f(r._h, None, p, p, None) == ERR_ARG
    assert f(r._h, p, None, p, None) == ERR_ARG
    assert f(r._h, p, p, None, None) == ERR_ARG
    assert f(None, None, None, None, None) == ERR_ARG
