"""rrx_search_longest_string / rrx_contains_string on a box without a device: the header declares them, the library exports them,
the Python and C++ layers reach them, and they refuse null arguments before any device call."""
import ctypes as C
import os
import re

import roaringregex_amd as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 2
NAMES = ("rrx_search_longest_string", "rrx_contains_string")


def test_the_header_declares_them_and_the_library_exports_them():
    hdr = open(os.path.join(ROOT, "include", "rrx.h")).read()
    assert re.search(r"^int rrx_search_longest_string\(const rrx_regex \*re, int device, const void \*d_bytes, size_t nbytes, uint64_t \*d_span, "
                     r"void \*stream\);$", hdr, re.M)
    assert re.search(r"^int rrx_contains_string\(const rrx_regex \*re, int device, const void \*d_bytes, size_t nbytes, uint8_t \*d_found, "
                     r"void \*stream\);$", hdr, re.M)
    lib = C.CDLL(os.path.join(ROOT, "roaringregex_amd", "librrx.so"))
    for name in NAMES:
        assert hasattr(lib, name) and name in rr.ABI_SYMBOLS
    assert hasattr(rr.RRegex, "search_longest_string") and hasattr(rr.RRegex, "contains_string")
    facade = open(os.path.join(ROOT, "include", "rregex.hpp")).read()
    assert re.search(r"void search_longest_string\(const void \*d_bytes, size_t nbytes, uint64_t \*d_span, void \*stream = nullptr\)", facade)
    assert re.search(r"void contains_string\(const void \*d_bytes, size_t nbytes, uint8_t \*d_found, void \*stream = nullptr\)", facade)
    assert "rrx_search_longest_string(f->handle()" in facade and "rrx_contains_string(f->handle()" in facade


def test_the_new_unit_is_in_the_build():
    mk = open(os.path.join(ROOT, "roaringregex_amd", "csrc", "Makefile")).read()
    assert re.search(r"^KERNELS = .*\bkernels_long_search\.hip\b", mk, re.M) and re.search(r"^HDRS .*\bkernels_long\.hpp\b", mk, re.M)


def test_null_arguments_are_refused_before_any_device_call():
    """(This box may have no device at all: a buffer of zeros stands for the device memory that cannot be made here.)"""
    r = rr.RRegex("ab+c")
    buf = (C.c_uint64 * 64)()
    p = C.cast(buf, C.c_void_p)
    for name in NAMES:
        f = getattr(rr._L, name)
        assert f(None, 0, p, 8, p, None) == ERR_ARG and b"null argument" in rr._L.rrx_last_error()
        assert f(r._h, 0, None, 8, p, None) == ERR_ARG            # no bytes, but a length
        assert f(r._h, 0, p, 8, None, None) == ERR_ARG
        assert f(r._h, 0, None, 0, None, None) == ERR_ARG          # the empty string still needs somewhere to answer
        assert f(None, 0, None, 0, None, None) == ERR_ARG
