"""rrx_bitmap_rank / rrx_filter_* on a box without a device: the header declares the seven entries with their exact signatures, the
library exports them, the Python surface is there, every entry refuses each null argument before any device call, the size of the
rank array follows its contract, and the Python rule (filter_cases.py) is what grep prints."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import roaringregex_amd as rr
from filter_cases import SCAN_CHUNK, corpus_cases, filter_rule, lines_of, pack_bits, rank_rule, selected_rows, sources_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 2

SIGNATURES = {
    "rrx_bitmap_rank_words": "size_t rrx_bitmap_rank_words(size_t nbits);",
    "rrx_bitmap_rank": "int rrx_bitmap_rank(int device, const uint32_t *d_bits, size_t nbits, int invert, uint64_t *d_rank, size_t rank_words, void *stream);",
    "rrx_filter_sizes": "int rrx_filter_sizes(int device, const uint64_t *d_off, size_t nitems, uint32_t trim, const uint32_t *d_bits, int invert, "
                        "const uint64_t *d_rank, uint64_t *d_row, uint32_t *d_piece_len, uint64_t *d_piece_src, void *stream);",
    "rrx_filter_corpus_sizes": "int rrx_filter_corpus_sizes(const rrx_corpus *c, const uint32_t *d_bits, int invert, int keep_newline, const uint64_t *d_rank, "
                               "uint64_t *d_row, uint32_t *d_piece_len, uint64_t *d_piece_src, void *stream);",
    "rrx_filter_contains_extents": "int rrx_filter_contains_extents(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, "
                                   "uint32_t trim, int invert, uint64_t *d_row, uint64_t *d_out_off, size_t rows_cap, void *d_out, size_t cap, size_t *nrows, "
                                   "size_t *total, void *stream);",
    "rrx_filter_contains_items": "int rrx_filter_contains_items(const rrx_regex *re, const rrx_items *items, int invert, uint64_t *d_row, uint64_t *d_out_off, "
                                 "size_t rows_cap, void *d_out, size_t cap, size_t *nrows, size_t *total, void *stream);",
    "rrx_filter_contains_corpus": "int rrx_filter_contains_corpus(const rrx_regex *re, const rrx_corpus *c, int invert, int keep_newline, uint64_t *d_row, "
                                  "uint64_t *d_out_off, size_t rows_cap, void *d_out, size_t cap, size_t *nrows, size_t *total, void *stream);",
}


def test_the_header_declares_the_seven_entries_and_the_library_exports_them():
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "rrx.h")).read())
    lib = C.CDLL(os.path.join(ROOT, "roaringregex_amd", "librrx.so"))
    for name, sig in SIGNATURES.items():
        assert sig in hdr, name
        assert hasattr(lib, name) and name in rr.ABI_SYMBOLS, name
    assert callable(rr.filter_rows) and hasattr(rr.Corpus, "filter_lines")
    for m in ("filter_contains_extents", "filter_contains_items", "filter_contains_corpus"):
        assert hasattr(rr.RRegex, m), m


def each_null(f, args, nullable=()):
    """f(*args) with each pointer argument (a c_void_p) in turn replaced by null is RRX_ERR_ARG; `nullable`: positions left out."""
    seen = 0
    for k, a in enumerate(args):
        if not isinstance(a, C.c_void_p) or k in nullable:
            continue
        call = list(args)
        call[k] = None
        assert f(*call) == ERR_ARG and b"null argument" in rr._L.rrx_last_error(), (f.__name__, k)
        seen += 1
    return seen


def private_library():
    """The library once more, with argument types of this test's own: every pointer a c_void_p, so that each can be null."""
    vp, sz, i32, u32 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32
    lib = C.CDLL(os.path.join(ROOT, "roaringregex_amd", "librrx.so"))
    tail = [vp, vp, sz, vp, sz, vp, vp, vp]                       # d_row, d_out_off, rows_cap, d_out, cap, nrows, total, stream
    for name, args in (("rrx_bitmap_rank", [i32, vp, sz, i32, vp, sz, vp]),
                       ("rrx_filter_sizes", [i32, vp, sz, u32, vp, i32, vp, vp, vp, vp, vp]),
                       ("rrx_filter_corpus_sizes", [vp, vp, i32, i32, vp, vp, vp, vp, vp]),
                       ("rrx_filter_contains_extents", [vp, i32, vp, vp, sz, u32, i32] + tail),
                       ("rrx_filter_contains_items", [vp, vp, i32] + tail),
                       ("rrx_filter_contains_corpus", [vp, vp, i32, i32] + tail)):
        f = getattr(lib, name)
        f.restype, f.argtypes = i32, args
    return lib


def test_null_arguments_are_refused_before_any_device_call():
    """(This box may have no device at all.  An entry looks at no argument before it has seen that all are there: a buffer of zeros
    stands for the arrays and for the handles that cannot be made here; the last argument, the stream, may be null.)"""
    L = private_library()
    buf = (C.c_uint64 * 64)()
    p = C.cast(buf, C.c_void_p)
    r = rr.RRegex("[0-9]+")
    re_h = C.c_void_p(r._h.value)
    assert each_null(L.rrx_bitmap_rank, [0, p, 5, 0, p, 64, None]) == 2
    assert each_null(L.rrx_filter_sizes, [0, p, 5, 0, p, 0, p, p, p, p, None]) == 6
    assert each_null(L.rrx_filter_corpus_sizes, [p, p, 0, 1, p, p, p, p, None]) == 6
    # (d_bytes may be null: the batch check of every _extents entry asks for the offsets)
    assert each_null(L.rrx_filter_contains_extents, [re_h, 0, p, p, 5, 0, 0, p, p, 5, p, 5, p, p, None], nullable=(2,)) == 7
    assert each_null(L.rrx_filter_contains_items, [re_h, p, 0, p, p, 5, p, 5, p, p, None]) == 7
    assert each_null(L.rrx_filter_contains_corpus, [re_h, p, 0, 1, p, p, 5, p, 5, p, p, None]) == 7
    assert L.rrx_bitmap_rank(0, None, 0, 0, None, 64, None) == ERR_ARG


def test_the_rank_array_has_room_for_its_entries_and_a_shorter_one_is_refused():
    L = rr._L
    buf = (C.c_uint64 * 64)()
    p = C.cast(buf, C.c_void_p)
    last = 0
    for n in list(range(0, 200)) + [2047, 2048, 2049, 32 * SCAN_CHUNK - 1, 32 * SCAN_CHUNK, 32 * SCAN_CHUNK + 1, 1 << 27, (1 << 27) + 1, 1 << 33]:
        w = L.rrx_bitmap_rank_words(n)
        assert w >= (n + 31) // 32 + 1 and w >= last, n
        last = w
        assert L.rrx_bitmap_rank(0, p, n, 0, p, w - 1, None) == ERR_ARG and b"rrx_bitmap_rank_words" in rr._L.rrx_last_error(), n
        assert L.rrx_bitmap_rank(0, p, n, 1, p, 0, None) == ERR_ARG, n


def test_the_rule_is_what_grep_prints():
    text = b"GET /a 200\n\nno digits\nerror 7\n\nlast line has 1 and no newline"
    rng = np.random.default_rng(3)
    for pattern in (rb"[0-9]+", rb"error|GET", rb"x*", rb"[^\x00-\xff]"):
        flags = [re.search(pattern, ln) is not None for ln, _ in lines_of(text)]
        bits = pack_bits(flags, rng)
        want = [ln for ln in text.split(b"\n") if re.search(pattern, ln)]
        rows, off, out = filter_rule(text, bits, False, False)
        assert [out[off[k]:off[k + 1]] for k in range(len(rows))] == want and list(rows) == [i for i, f in enumerate(flags) if f]
        # grep -v, the newlines kept: the other lines as they stand in the text
        rows, off, out = filter_rule(text, bits, True, True)
        others = [(ln, nl) for ln, nl in lines_of(text) if not re.search(pattern, ln)]
        assert out == b"".join(ln + (b"\n" if nl else b"") for ln, nl in others) and len(out) == off[-1]
        assert [text[s:s + 1] for s in sources_rule(text, bits, True)] == [ln[:1] or b"\n" for ln, _ in others]


def test_the_rule_on_items_and_spare_bits():
    items = [b"a\n", b"", b"\x00\xff", b"dd"]
    bits = np.array([0xFFFFFFF5], dtype=np.uint32)                 # rows 0 and 2; every spare bit set
    rows, off, out = filter_rule(items, bits, False)
    assert list(rows) == [0, 2] and list(off) == [0, 2, 4] and out == b"a\n\x00\xff"
    rows, off, out = filter_rule(items, bits, True)
    assert list(rows) == [1, 3] and list(off) == [0, 0, 2] and out == b"dd"
    assert list(rank_rule(bits, 4, False)) == [0, 2] and list(rank_rule(bits, 4, True)) == [0, 2] and list(rank_rule(bits, 0, True)) == [0]
    assert list(selected_rows(np.array([0, 0xFFFFFFFF], dtype=np.uint32), 33, True)) == list(range(32))
    rng = np.random.default_rng(9)
    for n in (1, 31, 32, 33, 95, 200):                             # the rank written word by word and the selection counted row by row agree
        words = rng.integers(0, 1 << 32, size=(n + 31) // 32, dtype=np.uint64).astype(np.uint32)
        for invert in (False, True):
            rows = selected_rows(words, n, invert)
            assert list(rank_rule(words, n, invert)) == [int((rows < 32 * w).sum()) for w in range((n + 31) // 32 + 1)]
    assert list(sources_rule(items, bits, False, first=5, trim=1)) == [5, 9]


@pytest.mark.parametrize("case", corpus_cases(), ids=lambda c: c[0])
def test_the_corpus_cases_are_texts_with_lines(case):
    name, text, extra = case
    n = len(lines_of(text))
    assert n and all(len(sel) == n for _, sel in extra), name
