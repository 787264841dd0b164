"""roaringregex_amd — MI355X-native engine for the RoaringRegex hot path.

Python host layer over the C ABI of librrx.so (include/rrx.h).  It mirrors the reference's interface for the
path (src/inc/regex.h:100-126, 212-228): RRegex(pattern), RRegex.get_acceptance_iter(text) ->
IteratorWrapper with advance() (the reference's operator++(int)) and value() (operator*, a Match or None),
plus the batch entry the reference lacks (Corpus / RRegex.match_corpus).  PyTorch is used only as plumbing
for device memory and streams.  There is no CPU matcher in this package: if librrx.so is missing the import
fails loudly, and matching without a gfx950 device raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.environ.get("RRX_LIB") or os.path.join(_HERE, "librrx.so")   # RRX_LIB: A/B builds of the same ABI

ENGINE_AUTO, ENGINE_NFA, ENGINE_DFA, ENGINE_DFA_GLOBAL, ENGINE_NFA_WAVE, ENGINE_DFA2 = 0, 1, 2, 3, 4, 5
PROGRAM_SEARCH_FWD, PROGRAM_SEARCH_REV = 6, 7          # rrx_program_words kinds of the two search tables
ENGINE_NFA_BLOCK = 8
ENGINE_NFA_SPARSE = 10
PROGRAM_SEARCH_LINE = 9
PROGRAM_SEARCH_LINE2 = 14
PROGRAM_DFA2_ITEMS = 15
PROGRAM_DFA2_ORDER = 11
PROGRAM_SAMPLED_DFA = 12
PROGRAM_SAMPLED_DFA2 = 13
PROGRAM_CONTAINS_DFA, PROGRAM_CONTAINS_DFA2 = 16, 17   # the contains table (rrx_contains_corpus) and its stride-2 form
PROGRAM_SEARCH_STARTS, PROGRAM_SEARCH_ANCHORED = 19, 20  # the two tables of the leftmost-longest search (rrx_search_longest_extents)
PROGRAM_CONTAINS_DFA2_ITEMS = 18                       # its stride-2 items form (rrx_contains_extents / rrx_contains_items, trim 1)
PROGRAM_GROUP_A, PROGRAM_GROUP_REV_BC, PROGRAM_GROUP_B, PROGRAM_GROUP_REV_C = 21, 22, 23, 24   # the four tables of an RGroup (rrx_group_program_words)
OPT_BACKGROUND_ORDER = 1
OPT_UNITS_PER_WORKGROUP = 2
OPT_SAMPLED_TABLE = 3
OPT_FLUSH_SLOTS = 4
OPT_SEARCH_ANCHORED = 5
OPT_ITEMS_STRIDE2 = 6
OPT_CONTAINS_NFA = 7                                    # contains on the NFA lane engine: 0 never, 1 where there is no table, 2 always
PROGRAM_CONTAINS_NFA = 25                               # the program it runs: the lane program with the contains B rows (NFA layout)

# every symbol include/rrx.h declares (tests check the library exports exactly these)
ABI_SYMBOLS = (
    "rrx_compile", "rrx_compile_ex", "rrx_free", "rrx_last_error",
    "rrx_num_states", "rrx_set_class", "rrx_ref_initial", "rrx_ref_is_final", "rrx_ref_row",
    "rrx_engine", "rrx_engine_name", "rrx_useful_states", "rrx_byte_classes", "rrx_table_order", "rrx_order_table", "rrx_set_option", "rrx_learn_table", "rrx_sampled_table", "rrx_sampled_escapes", "rrx_words_per_set", "rrx_accepts_empty",
    "rrx_program_words",
    "rrx_corpus_create", "rrx_corpus_create_ex", "rrx_corpus_stripe_bytes", "rrx_corpus_num_lines", "rrx_corpus_num_bytes", "rrx_corpus_free", "rrx_corpus_bitmap_words",
    "rrx_corpus_one_launch", "rrx_match_flush_slots",
    "rrx_match_corpus", "rrx_match_device", "rrx_search_corpus", "rrx_search_all_count", "rrx_search_all_fill", "rrx_search_all", "rrx_bitmap_to_bytes",
    "rrx_match_extents", "rrx_items_create", "rrx_items_count", "rrx_items_stripe_wise", "rrx_items_free", "rrx_match_items",
    "rrx_match_string", "rrx_match_host", "rrx_match_cstr", "rrx_search_longest_string", "rrx_contains_string",
    "rrx_contains_corpus", "rrx_contains_engine_name", "rrx_contains_states", "rrx_bitmap_count",
    "rrx_contains_extents", "rrx_contains_items",
    "rrx_search_extents", "rrx_search_items",
    "rrx_search_all_extents_count", "rrx_search_all_extents_fill", "rrx_search_all_extents",
    "rrx_search_all_items_count", "rrx_search_all_items_fill", "rrx_search_all_items",
    "rrx_search_longest_extents", "rrx_search_longest_items", "rrx_search_longest_corpus",
    "rrx_search_all_longest_marks_words",
    "rrx_search_all_longest_extents_count", "rrx_search_all_longest_extents_fill", "rrx_search_all_longest_extents",
    "rrx_search_all_longest_items_count", "rrx_search_all_longest_items_fill", "rrx_search_all_longest_items",
    "rrx_replace_matches_sizes", "rrx_replace_matches_fill", "rrx_replace_all_longest_extents", "rrx_replace_all_longest_items",
    "rrx_pieces_sizes", "rrx_pieces_fill", "rrx_extract_all_longest_extents", "rrx_extract_all_longest_items", "rrx_split_longest_extents",
    "rrx_split_longest_items",
    "rrx_bitmap_rank_words", "rrx_bitmap_rank", "rrx_filter_sizes", "rrx_filter_corpus_sizes",
    "rrx_filter_contains_extents", "rrx_filter_contains_items", "rrx_filter_contains_corpus",
    "rrx_group_compile", "rrx_group_compile_ex", "rrx_group_free", "rrx_group_regex", "rrx_group_part", "rrx_group_program_words",
    "rrx_group_spans_extents", "rrx_group_spans_items", "rrx_extract_group_longest_extents", "rrx_extract_group_longest_items",
    "rrx_group_spans_list_extents", "rrx_group_spans_list_items",
    "rrx_template_compile", "rrx_template_free", "rrx_template_refs", "rrx_template_segments",
    "rrx_replace_template_sizes", "rrx_replace_template_fill", "rrx_replace_groups_longest_extents", "rrx_replace_groups_longest_items",
    "rrx_multi_compile", "rrx_multi_compile_ex", "rrx_multi_free", "rrx_multi_patterns", "rrx_multi_groups", "rrx_multi_group_mask",
    "rrx_multi_group_states", "rrx_multi_program_words", "rrx_multi_contains_extents", "rrx_multi_contains_items", "rrx_multi_contains_corpus",
    "rrx_multi_counts", "rrx_multi_plane",
)


class RRegexError(RuntimeError):
    """The reference throws std::runtime_error (Parser.cpp:36,155); so do we."""


def _load():
    if not os.path.exists(_SO):
        raise ImportError(
            "roaringregex_amd: %s is missing — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback." % _SO)
    # librrx.so needs libamdhip64.so.7.  PyTorch-ROCm ships its own copy under the same SONAME and the dynamic
    # loader keeps whichever is loaded first, so import torch first: one HIP runtime per process, the one that
    # owns the tensors we are handed.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(_SO)
    vp, u32, sz, i32 = C.c_void_p, C.c_uint32, C.c_size_t, C.c_int
    sig = {
        "rrx_compile": (i32, [C.c_char_p, C.POINTER(vp)]),
        "rrx_compile_ex": (i32, [C.c_char_p, i32, C.POINTER(vp)]),
        "rrx_free": (None, [vp]),
        "rrx_last_error": (C.c_char_p, []),
        "rrx_num_states": (u32, [vp]),
        "rrx_set_class": (i32, [vp]),
        "rrx_ref_initial": (u32, [vp]),
        "rrx_ref_is_final": (i32, [vp, u32]),
        "rrx_ref_row": (u32, [vp, u32, C.c_uint, vp, u32]),
        "rrx_engine": (i32, [vp]),
        "rrx_engine_name": (C.c_char_p, [vp]),
        "rrx_useful_states": (u32, [vp]),
        "rrx_byte_classes": (u32, [vp]),
        "rrx_table_order": (i32, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "rrx_set_option": (i32, [vp, i32, C.c_int64]),
        "rrx_learn_table": (i32, [vp, vp, C.c_size_t]),
        "rrx_sampled_table": (i32, [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "rrx_sampled_escapes": (i32, [vp, i32, C.POINTER(C.c_uint64)]),
        "rrx_order_table": (i32, [vp, vp, u32, u32]),
        "rrx_words_per_set": (u32, [vp]),
        "rrx_accepts_empty": (i32, [vp]),
        "rrx_program_words": (sz, [vp, i32, vp, sz]),
        "rrx_corpus_create": (i32, [i32, vp, sz, vp, C.POINTER(vp)]),
        "rrx_corpus_create_ex": (i32, [i32, vp, sz, u32, vp, C.POINTER(vp)]),
        "rrx_corpus_stripe_bytes": (u32, [vp]),
        "rrx_corpus_num_lines": (sz, [vp]),
        "rrx_corpus_num_bytes": (sz, [vp]),
        "rrx_corpus_free": (None, [vp]),
        "rrx_corpus_bitmap_words": (sz, [vp]),
        "rrx_corpus_one_launch": (i32, [vp, C.POINTER(u32)]),
        "rrx_match_flush_slots": (u32, [vp, vp, C.POINTER(i32)]),
        "rrx_match_corpus": (i32, [vp, vp, vp, vp]),
        "rrx_match_device": (i32, [vp, i32, vp, sz, vp, sz, C.POINTER(sz), vp]),
        "rrx_bitmap_to_bytes": (i32, [i32, vp, sz, vp, vp]),
        "rrx_match_extents": (i32, [vp, i32, vp, vp, sz, u32, vp, vp]),
        "rrx_items_create": (i32, [i32, vp, vp, sz, u32, vp, C.POINTER(vp)]),
        "rrx_items_count": (sz, [vp]),
        "rrx_items_stripe_wise": (i32, [vp]),
        "rrx_items_free": (None, [vp]),
        "rrx_match_items": (i32, [vp, vp, vp, vp]),
        "rrx_match_string": (i32, [vp, i32, vp, sz, vp, vp]),
        "rrx_search_longest_string": (i32, [vp, i32, vp, sz, vp, vp]),
        "rrx_contains_string": (i32, [vp, i32, vp, sz, vp, vp]),
        "rrx_search_corpus": (i32, [vp, vp, vp, vp, vp]),
        "rrx_search_all_count": (i32, [vp, vp, vp, vp]),
        "rrx_search_all_fill": (i32, [vp, vp, vp, vp, vp, vp]),
        "rrx_search_all": (i32, [vp, vp, vp, vp, vp, sz, C.POINTER(sz), vp]),
        "rrx_match_host": (i32, [vp, i32, vp, sz, vp, sz, C.POINTER(sz)]),
        "rrx_match_cstr": (i32, [vp, i32, C.c_char_p, C.POINTER(i32), C.POINTER(sz)]),
        "rrx_contains_corpus": (i32, [vp, vp, vp, vp]),
        "rrx_contains_engine_name": (C.c_char_p, [vp]),
        "rrx_contains_states": (u32, [vp]),
        "rrx_bitmap_count": (i32, [i32, vp, sz, vp, vp]),
        "rrx_contains_extents": (i32, [vp, i32, vp, vp, sz, u32, vp, vp]),
        "rrx_contains_items": (i32, [vp, vp, vp, vp]),
        "rrx_search_extents": (i32, [vp, i32, vp, vp, sz, u32, vp, vp, vp]),
        "rrx_search_items": (i32, [vp, vp, vp, vp, vp]),
        "rrx_search_all_extents_count": (i32, [vp, i32, vp, vp, sz, u32, vp, vp]),
        "rrx_search_all_extents_fill": (i32, [vp, i32, vp, vp, sz, u32, vp, vp, vp, vp]),
        "rrx_search_all_extents": (i32, [vp, i32, vp, vp, sz, u32, vp, vp, vp, sz, C.POINTER(sz), vp]),
        "rrx_search_all_items_count": (i32, [vp, vp, vp, vp]),
        "rrx_search_all_items_fill": (i32, [vp, vp, vp, vp, vp, vp]),
        "rrx_search_all_items": (i32, [vp, vp, vp, vp, vp, sz, C.POINTER(sz), vp]),
        "rrx_search_longest_extents": (i32, [vp, i32, vp, vp, sz, u32, vp, vp, vp]),
        "rrx_search_longest_items": (i32, [vp, vp, vp, vp, vp]),
        "rrx_search_longest_corpus": (i32, [vp, vp, vp, vp, vp]),
        "rrx_search_all_longest_marks_words": (sz, [sz, sz]),
        "rrx_search_all_longest_extents_count": (i32, [vp, i32, vp, vp, sz, u32, vp, sz, vp, vp]),
        "rrx_search_all_longest_extents_fill": (i32, [vp, i32, vp, vp, sz, u32, vp, sz, vp, vp, vp, vp]),
        "rrx_search_all_longest_extents": (i32, [vp, i32, vp, vp, sz, u32, vp, vp, vp, sz, C.POINTER(sz), vp]),
        "rrx_search_all_longest_items_count": (i32, [vp, vp, vp, sz, vp, vp]),
        "rrx_search_all_longest_items_fill": (i32, [vp, vp, vp, sz, vp, vp, vp, vp]),
        "rrx_search_all_longest_items": (i32, [vp, vp, vp, vp, vp, sz, C.POINTER(sz), vp]),
        "rrx_replace_matches_sizes": (i32, [i32, vp, sz, u32, vp, vp, vp, u32, vp, vp, vp]),
        "rrx_replace_matches_fill": (i32, [i32, vp, vp, sz, u32, vp, vp, vp, vp, u32, vp, vp, vp]),
        "rrx_replace_all_longest_extents": (i32, [vp, i32, vp, vp, sz, u32, vp, u32, vp, vp, sz, C.POINTER(sz), vp]),
        "rrx_replace_all_longest_items": (i32, [vp, vp, vp, u32, vp, vp, sz, C.POINTER(sz), vp]),
        "rrx_pieces_sizes": (i32, [i32, vp, sz, u32, vp, vp, vp, i32, vp, vp, vp, vp]),
        "rrx_pieces_fill": (i32, [i32, vp, vp, vp, sz, vp, vp]),
        "rrx_extract_all_longest_extents": (i32, [vp, i32, vp, vp, sz, u32, vp, vp, sz, vp, sz, C.POINTER(sz), C.POINTER(sz), vp]),
        "rrx_extract_all_longest_items": (i32, [vp, vp, vp, vp, sz, vp, sz, C.POINTER(sz), C.POINTER(sz), vp]),
        "rrx_split_longest_extents": (i32, [vp, i32, vp, vp, sz, u32, vp, vp, sz, vp, sz, C.POINTER(sz), C.POINTER(sz), vp]),
        "rrx_split_longest_items": (i32, [vp, vp, vp, vp, sz, vp, sz, C.POINTER(sz), C.POINTER(sz), vp]),
        "rrx_bitmap_rank_words": (sz, [sz]),
        "rrx_bitmap_rank": (i32, [i32, vp, sz, i32, vp, sz, vp]),
        "rrx_filter_sizes": (i32, [i32, vp, sz, u32, vp, i32, vp, vp, vp, vp, vp]),
        "rrx_filter_corpus_sizes": (i32, [vp, vp, i32, i32, vp, vp, vp, vp, vp]),
        "rrx_filter_contains_extents": (i32, [vp, i32, vp, vp, sz, u32, i32, vp, vp, sz, vp, sz, C.POINTER(sz), C.POINTER(sz), vp]),
        "rrx_filter_contains_items": (i32, [vp, vp, i32, vp, vp, sz, vp, sz, C.POINTER(sz), C.POINTER(sz), vp]),
        "rrx_filter_contains_corpus": (i32, [vp, vp, i32, i32, vp, vp, sz, vp, sz, C.POINTER(sz), C.POINTER(sz), vp]),
        "rrx_group_compile": (i32, [C.c_char_p, i32, C.POINTER(vp)]),
        "rrx_group_compile_ex": (i32, [C.c_char_p, i32, i32, C.POINTER(vp)]),
        "rrx_group_free": (None, [vp]),
        "rrx_group_regex": (vp, [vp]),
        "rrx_group_part": (sz, [vp, i32, vp, sz]),
        "rrx_group_program_words": (sz, [vp, i32, vp, sz]),
        "rrx_group_spans_extents": (i32, [vp, i32, vp, vp, sz, u32, vp, vp, vp, sz, vp, vp, vp]),
        "rrx_group_spans_items": (i32, [vp, vp, vp, vp, vp, sz, vp, vp, vp]),
        "rrx_extract_group_longest_extents": (i32, [vp, i32, vp, vp, sz, u32, vp, sz, vp, vp, vp]),
        "rrx_extract_group_longest_items": (i32, [vp, vp, vp, sz, vp, vp, vp]),
        "rrx_group_spans_list_extents": (i32, [vp, i32, vp, vp, sz, u32, vp, vp, vp, vp, sz, vp, vp, vp]),
        "rrx_group_spans_list_items": (i32, [vp, vp, vp, vp, vp, vp, sz, vp, vp, vp]),
        "rrx_template_compile": (i32, [vp, sz, C.POINTER(vp)]),
        "rrx_template_free": (None, [vp]),
        "rrx_template_refs": (sz, [vp, vp, sz]),
        "rrx_template_segments": (sz, [vp, vp, vp, sz, vp, sz]),
        "rrx_replace_template_sizes": (i32, [i32, vp, sz, u32, vp, vp, vp, vp, vp, vp, sz, vp, vp, vp]),
        "rrx_replace_template_fill": (i32, [i32, vp, vp, sz, u32, vp, vp, vp, vp, vp, vp, vp, sz, vp, vp, vp]),
        "rrx_replace_groups_longest_extents": (i32, [vp, sz, vp, i32, vp, vp, sz, u32, vp, vp, sz, C.POINTER(sz), vp]),
        "rrx_replace_groups_longest_items": (i32, [vp, sz, vp, vp, vp, vp, sz, C.POINTER(sz), vp]),
        "rrx_multi_compile": (i32, [vp, sz, C.POINTER(vp)]),
        "rrx_multi_compile_ex": (i32, [vp, sz, i32, u32, C.POINTER(vp)]),
        "rrx_multi_free": (None, [vp]),
        "rrx_multi_patterns": (sz, [vp]),
        "rrx_multi_groups": (sz, [vp]),
        "rrx_multi_group_mask": (u32, [vp, sz]),
        "rrx_multi_group_states": (u32, [vp, sz]),
        "rrx_multi_program_words": (sz, [vp, sz, vp, sz]),
        "rrx_multi_contains_extents": (i32, [vp, i32, vp, vp, sz, u32, vp, vp]),
        "rrx_multi_contains_items": (i32, [vp, vp, vp, vp]),
        "rrx_multi_contains_corpus": (i32, [vp, vp, vp, vp]),
        "rrx_multi_counts": (i32, [i32, vp, sz, vp, vp]),
        "rrx_multi_plane": (i32, [i32, vp, sz, u32, vp, vp]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    return L


_L = _load()


def _check(rc):
    if rc != 0:
        raise RRegexError(_L.rrx_last_error().decode("latin-1"))


class _on:
    """Run a method body on `device` and, when the caller names a stream, with that stream as torch's CURRENT stream:
    the tensors the body allocates, torch ops such as cumsum/item and the native launches then all live on one stream
    (the native calls are handed the same stream by _stream_ptr)."""

    def __init__(self, device, stream):
        import torch
        self._dev = torch.cuda.device(device)
        self._st = torch.cuda.stream(stream) if stream is not None else None

    def __enter__(self):
        self._dev.__enter__()
        if self._st is not None:
            self._st.__enter__()

    def __exit__(self, *exc):
        if self._st is not None:
            self._st.__exit__(*exc)
        return self._dev.__exit__(*exc)


def _stream_ptr(stream):
    if stream is None:
        import torch
        stream = torch.cuda.current_stream()
    return C.c_void_p(stream.cuda_stream)


def bitmap_count(bits, nlines, stream=None):
    """Set bits among the first `nlines` bits of a result bitmap (a device tensor of 32-bit words, as match_corpus_bits and
    contains_corpus_bits return it), counted on the device (rrx_bitmap_count) -> int.  Waits for the one word to come back."""
    import torch
    assert bits.is_cuda and bits.dtype in (torch.int32, torch.uint32) and bits.is_contiguous() and bits.numel() * 32 >= nlines
    with _on(bits.device.index, stream):
        count = torch.empty(1, dtype=torch.int64, device=bits.device)
        _check(_L.rrx_bitmap_count(bits.device.index, _ptr(bits[:(nlines + 31) // 32]), nlines, C.c_void_p(count.data_ptr()),
                                   _stream_ptr(stream)))
        return int(count.item())


def _ptr(t):
    """The address of a tensor's first element, or null for an empty one."""
    return C.c_void_p(t.data_ptr() if t.numel() else 0)


def _batch(data, offsets):
    """A batch of items nobody has indexed, as every _extents method takes it: item i = data[offsets[i] : offsets[i + 1] - trim] ->
    (n, the device's index, the address of the bytes, the address of the offsets)."""
    import torch
    assert data.is_cuda and data.dtype == torch.uint8 and offsets.is_cuda and offsets.dtype in (torch.int64, torch.uint64) and offsets.is_contiguous()
    return offsets.numel() - 1, data.device.index, _ptr(data), C.c_void_p(offsets.data_ptr())


def _span_pair(n, device):
    """The (start, end) outputs of a search: two int32 tensors of n entries."""
    import torch
    return torch.empty(n, dtype=torch.int32, device=device), torch.empty(n, dtype=torch.int32, device=device)


def _out(out, n, dtype, device):
    """The output of an entry that writes n words of `dtype`: a fresh tensor, or the caller's `out` - on the device, of that dtype,
    contiguous, n entries at least - cut to n."""
    import torch
    if out is None:
        return torch.empty(n, dtype=dtype, device=device)
    assert out.is_cuda and out.dtype == dtype and out.is_contiguous() and out.numel() >= n
    return out[:n]


def _bits_to_bytes(bits, n, out, device, stream):
    """One byte per bit of the first n bits of a result bitmap (rrx_bitmap_to_bytes), into `out` as _out takes it."""
    import torch
    out = _out(out, n, torch.uint8, device)
    _check(_L.rrx_bitmap_to_bytes(device.index, _ptr(bits), n, _ptr(out), _stream_ptr(stream)))
    return out


def _check_match_list(n, first, start, end):
    """What every entry on a match list asks of it: `first` with n + 1 entries, start and end of one length."""
    import torch
    assert first.is_cuda and first.dtype in (torch.int64, torch.uint64) and first.is_contiguous() and first.numel() == n + 1
    assert all(t.is_cuda and t.dtype in (torch.int32, torch.uint32) and t.is_contiguous() for t in (start, end)) and start.numel() == end.numel()


def _no_null(start, end, device):
    """(start, end), or one word in place of both where they are empty or not there: the entries take no null array, even where the
    lists are empty."""
    import torch
    if start is not None and start.numel():
        return start, end
    word = torch.zeros(1, dtype=torch.int32, device=device)
    return word, word


def _offsets_and_bytes(length, device):
    """From the lengths of a column's entries (32-bit words, unsigned whatever the dtype says) to its offsets and its bytes ->
    (out_off int64[n + 1], out uint8[total], uninitialised).  Waits for the total."""
    import torch
    out_off = torch.zeros(length.numel() + 1, dtype=torch.int64, device=device)
    torch.cumsum(length.to(torch.int64) & 0xFFFFFFFF, dim=0, out=out_off[1:])
    return out_off, torch.empty(int(out_off[-1].item()), dtype=torch.uint8, device=device)


def _retry(caps, alloc, call):
    """A one-call entry, repeated with the exact sizes if a cap was too small: alloc(*caps) -> the output tensors, call(tensors, caps)
    -> the sizes the entry reports, one per cap.  Each cap grows to the reported size.  -> (the tensors, the sizes)"""
    while True:
        bufs = alloc(*caps)
        need = call(bufs, caps)
        if all(x <= c for x, c in zip(need, caps)):
            return bufs, need
        caps = tuple(max(c, x) for x, c in zip(need, caps))


def _search_all_two_pass(dev, n, count_call, fill_call):
    """count, the prefix with torch, fill -> (count, first, start, end), as search_all shapes them."""
    import torch
    count = torch.zeros(n, dtype=torch.int32, device=dev)
    _check(count_call(_ptr(count)))
    inclusive = torch.cumsum(count, dim=0, dtype=torch.int64)
    first = inclusive - count
    start, end = _span_pair(int(inclusive[-1].item()) if n else 0, dev)
    if start.numel():
        _check(fill_call(C.c_void_p(first.data_ptr()), C.c_void_p(start.data_ptr()), C.c_void_p(end.data_ptr())))
    return count, first, start, end


def _search_all_one_call(dev, n, cap, call):
    """The one-call entry, repeated with the exact size if `cap` was too small -> (first[n + 1], start, end)."""
    import torch
    first = torch.empty(n + 1, dtype=torch.int64, device=dev)

    def run(bufs, caps):
        total = C.c_size_t(0)
        _check(call(C.c_void_p(first.data_ptr()), _ptr(bufs[0]), _ptr(bufs[1]), caps[0], C.byref(total)))
        return (total.value,)
    (start, end), (total,) = _retry((int(cap) if cap is not None else 2 * n + 1024,), lambda c: _span_pair(c, dev), run)
    return first, start[:total], end[:total]


def _replace_one_call(dev, n, cap, call):
    """The one-call replace entry, repeated with the exact size if `cap` was too small -> (out uint8, out_off int64[n + 1])."""
    import torch
    out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)

    def run(bufs, caps):
        total = C.c_size_t(0)
        _check(call(_ptr(out_off), _ptr(bufs[0]), caps[0], C.byref(total)))
        return (total.value,)
    (out,), (total,) = _retry((cap,), lambda c: (torch.empty(c, dtype=torch.uint8, device=dev),), run)
    return out[:total], out_off


def _pieces_one_call(dev, n, nbytes, cap, pieces_cap, call):
    """A one-call pieces entry, repeated with the exact sizes if a cap was too small -> (out, piece_off[npieces + 1], list_off[n + 1])."""
    import torch
    list_off = torch.empty(n + 1, dtype=torch.int64, device=dev)

    def run(bufs, caps):
        npieces, total = C.c_size_t(0), C.c_size_t(0)
        _check(call(_ptr(list_off), _ptr(bufs[1]), caps[1], _ptr(bufs[0]), caps[0], C.byref(npieces), C.byref(total)))
        return total.value, npieces.value
    caps = (int(cap) if cap is not None else nbytes, int(pieces_cap) if pieces_cap is not None else 2 * n)
    (out, piece_off), (total, npieces) = _retry(caps, lambda c, pc: (torch.empty(c, dtype=torch.uint8, device=dev),
                                                                     torch.empty(pc + 1, dtype=torch.int64, device=dev)), run)
    return out[:total], piece_off[:npieces + 1], list_off


def _filter_one_call(dev, n, nbytes, cap, rows_cap, call):
    """A one-call filter entry, repeated with the exact sizes if a cap was too small -> (rows int64[nrows], out_off int64[nrows + 1], out uint8)."""
    import torch

    def run(bufs, caps):
        nrows, total = C.c_size_t(0), C.c_size_t(0)
        _check(call(_ptr(bufs[1]), _ptr(bufs[2]), caps[1], _ptr(bufs[0]), caps[0], C.byref(nrows), C.byref(total)))
        return total.value, nrows.value
    caps = (int(cap) if cap is not None else nbytes, int(rows_cap) if rows_cap is not None else n)
    (out, rows, out_off), (total, nrows) = _retry(caps, lambda c, rc: (torch.empty(c, dtype=torch.uint8, device=dev),
                                                                       torch.empty(rc, dtype=torch.int64, device=dev),
                                                                       torch.empty(rc + 1, dtype=torch.int64, device=dev)), run)
    return rows[:nrows], out_off[:nrows + 1], out[:total]


def replace_matches(data, offsets, first, start, end, repl, trim=0, stream=None):
    """regexp_replace from a match list, written on the device (rrx_replace_matches_sizes, a torch.cumsum, rrx_replace_matches_fill):
    item i = data[offsets[i] : offsets[i + 1] - trim]; its matches are start/end[first[i] : first[i + 1]], relative to the item, as
    every search_all*_fused method returns them (`first` has n + 1 entries); `repl` is bytes, a literal.  -> (out uint8,
    out_off int64[n + 1]): output item i = out[out_off[i] : out_off[i + 1]], the item with every match replaced by `repl`; the
    separators are not copied.  The lists need not come from a regex of this library.  Waits for the output's size."""
    import torch
    n, d = _batch(data, offsets)[:2]
    _check_match_list(n, first, start, end)
    assert isinstance(repl, (bytes, bytearray))
    with _on(d, stream):
        s = _stream_ptr(stream)
        start, end = _no_null(start, end, data.device)
        length = torch.empty(n, dtype=torch.int32, device=data.device)
        pos = torch.empty(start.numel(), dtype=torch.int32, device=data.device)
        _check(_L.rrx_replace_matches_sizes(d, _ptr(offsets), n, trim, _ptr(first), _ptr(start), _ptr(end), len(repl), _ptr(length), _ptr(pos), s))
        out_off, out = _offsets_and_bytes(length, data.device)
        rep = torch.frombuffer(bytearray(repl), dtype=torch.uint8).to(data.device) if repl else torch.empty(0, dtype=torch.uint8, device=data.device)
        _check(_L.rrx_replace_matches_fill(d, _ptr(data), _ptr(offsets), n, trim, _ptr(first), _ptr(end), _ptr(pos), _ptr(rep), len(repl), _ptr(out_off),
                                           _ptr(out), s))
    return out, out_off


class Template:
    """A replacement with group references (rrx_template): bytes are literal except b"\\": \\0 ... \\9 is a reference (0 the whole
    match, one digit: \\12 is group 1 and a literal 2), \\\\ one backslash; anything else behind a backslash raises RRegexError with
    the offset.  At most 32 segments.  Template(rb"\\3-\\1-\\2").refs == (1, 2, 3)."""

    def __init__(self, repl):
        if isinstance(repl, str):
            repl = repl.encode("latin-1")
        assert isinstance(repl, (bytes, bytearray))
        self.repl = bytes(repl)
        self._h = C.c_void_p()
        _check(_L.rrx_template_compile(self.repl, len(self.repl), C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None) and _L is not None:
            _L.rrx_template_free(self._h)
            self._h = None

    @property
    def refs(self):
        """The distinct referenced groups >= 1, ascending: the r-th is plane r of replace_template."""
        n = _L.rrx_template_refs(self._h, None, 0)
        out = (C.c_int * max(n, 1))()
        _L.rrx_template_refs(self._h, out, n)
        return tuple(out[:n])

    @property
    def segments(self):
        """The segments in order: bytes for a literal, an int for a reference."""
        n = _L.rrx_template_segments(self._h, None, None, 0, None, 0)
        refs, lens, lits = (C.c_int * max(n, 1))(), (C.c_uint32 * max(n, 1))(), C.create_string_buffer(max(len(self.repl), 1))
        _L.rrx_template_segments(self._h, refs, lens, n, lits, len(self.repl))
        out, at = [], 0
        for k in range(n):
            if refs[k] < 0:
                out.append(lits.raw[at:at + lens[k]])
                at += lens[k]
            else:
                out.append(int(refs[k]))
        return tuple(out)


def replace_template(data, offsets, first, start, end, template, ref_start=None, ref_end=None, plane_stride=None, trim=0, stream=None):
    """replace_matches with a Template in place of the literal (rrx_replace_template_sizes, a torch.cumsum, rrx_replace_template_fill):
    ref_start / ref_end hold the span of plane r (the r-th of template.refs) in slot q at index r * plane_stride + q, relative to the
    item, -1 for "none" - for example RGroup.spans_list_extents' outputs, one group behind the other; plane_stride defaults to
    start.numel().  They may be left out when the template references no group >= 1.  -> (out uint8, out_off int64[n + 1]).  Waits
    for the output's size."""
    import torch
    n, d = _batch(data, offsets)[:2]
    assert isinstance(template, Template)
    _check_match_list(n, first, start, end)
    nrefs = len(template.refs)
    stride = int(plane_stride) if plane_stride is not None else start.numel()
    if nrefs:
        assert all(t is not None and t.is_cuda and t.dtype in (torch.int32, torch.uint32) and t.is_contiguous() for t in (ref_start, ref_end))
        assert stride >= start.numel() and min(ref_start.numel(), ref_end.numel()) >= (nrefs - 1) * stride + start.numel()
    with _on(d, stream):
        s = _stream_ptr(stream)
        start, end = _no_null(start, end, data.device)
        ref_start, ref_end = _no_null(ref_start if nrefs else None, ref_end, data.device)
        length = torch.empty(n, dtype=torch.int32, device=data.device)
        pos = torch.empty(start.numel(), dtype=torch.int32, device=data.device)
        _check(_L.rrx_replace_template_sizes(d, _ptr(offsets), n, trim, _ptr(first), _ptr(start), _ptr(end), template._h, _ptr(ref_start), _ptr(ref_end),
                                             stride, _ptr(length), _ptr(pos), s))
        out_off, out = _offsets_and_bytes(length, data.device)
        _check(_L.rrx_replace_template_fill(d, _ptr(data), _ptr(offsets), n, trim, _ptr(first), _ptr(start), _ptr(end), _ptr(pos), template._h,
                                            _ptr(ref_start), _ptr(ref_end), stride, _ptr(out_off), _ptr(out), s))
    return out, out_off


PIECES_MATCHES, PIECES_GAPS = 0, 1


def pieces_of_matches(data, offsets, first, start, end, gaps=False, trim=0, stream=None):
    """regexp_extract_all (gaps=False) or split (gaps=True) from a match list, written on the device as a list<binary> column
    (rrx_pieces_sizes, a torch.cumsum, rrx_pieces_fill): item i = data[offsets[i] : offsets[i + 1] - trim]; its matches are
    start/end[first[i] : first[i + 1]], relative to the item, as every search_all*_fused method returns them (`first` has n + 1
    entries).  -> (out uint8, piece_off int64[npieces + 1], list_off int64[n + 1]): the pieces of item i are list_off[i] ..
    list_off[i + 1], piece p = out[piece_off[p] : piece_off[p + 1]] - the matches themselves, or what lies between them (one more
    than the matches: re.split).  The lists need not come from a regex of this library.  Waits for the output's size."""
    import torch
    n, d = _batch(data, offsets)[:2]
    _check_match_list(n, first, start, end)
    with _on(d, stream):
        s = _stream_ptr(stream)
        list_off = torch.zeros(n + 1, dtype=torch.int64, device=data.device)
        if not n:
            return torch.empty(0, dtype=torch.uint8, device=data.device), torch.zeros(1, dtype=torch.int64, device=data.device), list_off
        npieces = int((first[-1] - first[0]).item()) + (n if gaps else 0)
        start, end = _no_null(start, end, data.device)
        length = torch.empty(max(npieces, 1), dtype=torch.int32, device=data.device)
        src = torch.empty(max(npieces, 1), dtype=torch.int64, device=data.device)
        _check(_L.rrx_pieces_sizes(d, _ptr(offsets), n, trim, _ptr(first), _ptr(start), _ptr(end), PIECES_GAPS if gaps else PIECES_MATCHES, _ptr(list_off),
                                   _ptr(length), _ptr(src), s))
        piece_off, out = _offsets_and_bytes(length[:npieces], data.device)
        _check(_L.rrx_pieces_fill(d, _ptr(data), _ptr(src), _ptr(piece_off), npieces, _ptr(out), s))
    return out, piece_off, list_off


def _filter_rank(bits, n, invert, dev, s):
    """rrx_bitmap_rank of the first n bits of a result bitmap -> (the rank array, the number of selected rows).  Waits for the one word."""
    import torch
    nw = (n + 31) // 32
    assert bits.is_cuda and bits.dtype in (torch.int32, torch.uint32) and bits.is_contiguous() and bits.numel() >= nw
    words = _L.rrx_bitmap_rank_words(n)
    rank = torch.empty(words, dtype=torch.int64, device=bits.device)
    _check(_L.rrx_bitmap_rank(dev, _ptr(bits), n, int(bool(invert)), _ptr(rank), words, s))
    return rank, int(rank[nw].item())


def _filter_column(data, nsel, sizes, dev, s):
    """The selected rows' triples (sizes(rows, length, src): one of the two generic entries), a torch.cumsum and rrx_pieces_fill ->
    (rows int64[nsel], out_off int64[nsel + 1], out uint8).  Waits for the output's size."""
    import torch
    rows = torch.empty(nsel, dtype=torch.int64, device=data.device)
    if not nsel:
        return rows, torch.zeros(1, dtype=torch.int64, device=data.device), torch.empty(0, dtype=torch.uint8, device=data.device)
    length = torch.empty(nsel, dtype=torch.int32, device=data.device)
    src = torch.empty(nsel, dtype=torch.int64, device=data.device)
    _check(sizes(_ptr(rows), _ptr(length), _ptr(src)))
    out_off, out = _offsets_and_bytes(length, data.device)
    _check(_L.rrx_pieces_fill(dev, _ptr(data), _ptr(src), _ptr(out_off), nsel, _ptr(out), s))
    return rows, out_off, out


def filter_rows(data, offsets, bits, invert=False, trim=0, stream=None):
    """The items a result bitmap selects, as a new column written on the device (rrx_bitmap_rank, rrx_filter_sizes, a torch.cumsum,
    rrx_pieces_fill): item i = data[offsets[i] : offsets[i + 1] - trim] is selected iff bit i & 31 of bits[i >> 5] is 1 (invert: 0);
    `bits` is what contains_extents_bits, contains_items_bits and RMulti.plane return, or any bitmap in that layout - the bits of
    its last word beyond the last item are ignored.  -> (rows int64[nsel], out_off int64[nsel + 1], out uint8): rows[k] is the
    number of the k-th selected item and out[out_off[k] : out_off[k + 1]] its bytes; the separators are not copied.  Waits for the
    number of rows and for the output's size."""
    n, d = _batch(data, offsets)[:2]
    with _on(d, stream):
        s = _stream_ptr(stream)
        rank, nsel = _filter_rank(bits, n, invert, d, s)
        return _filter_column(data, nsel, lambda rows, length, src: _L.rrx_filter_sizes(d, _ptr(offsets), n, trim, _ptr(bits), int(bool(invert)), _ptr(rank), rows,
                                                                                        length, src, s), d, s)


class Match:
    """regex.h:100-105: [start, end) into the caller's buffer; here as offsets plus the buffer."""

    def __init__(self, buf, start, end):
        self._buf, self.start, self.end = buf, start, end

    def str(self):
        return self._buf[self.start:self.end]


class IteratorWrapper:
    """regex.h:113-122 / 150-165.  advance() = operator++(int): consume the whole string (idempotent
    afterwards); value() = operator*: Match or None.  Before advance() the state set is {initial}."""

    def __init__(self, regex, text, device):
        self._re, self._text, self._device = regex, text, device
        self._consumed = False
        self._accepted = None

    def advance(self):
        if not self._consumed:
            acc, n = C.c_int(0), C.c_size_t(0)
            _check(_L.rrx_match_cstr(self._re._h, self._device, self._text, C.byref(acc), C.byref(n)))
            self._accepted, self._len = bool(acc.value), n.value
            self._consumed = True
        return self

    def value(self):
        if not self._consumed:
            # NFA.cc:103-107 on the initial set: only patterns whose initial state is final accept here
            return Match(self._text, 0, 0) if self._re.accepts_empty else None
        return Match(self._text, 0, self._len) if self._accepted else None

    def create_copy(self):
        c = IteratorWrapper(self._re, self._text, self._device)
        c.__dict__.update(self.__dict__)
        return c


class Corpus:
    """A device-resident batch of '\\n'-delimited strings plus its per-tile newline index (rrx_corpus)."""

    def __init__(self, data, device=None, stream=None, stripe=0):
        import torch
        if isinstance(data, (bytes, bytearray, memoryview)):
            data = torch.frombuffer(bytearray(data), dtype=torch.uint8) if len(data) else torch.empty(0, dtype=torch.uint8)
        if not data.is_cuda:
            dev = torch.device("cuda", 0 if device is None else device)
            data = data.to(dev)
        assert data.dtype == torch.uint8 and data.is_contiguous()
        self.data = data                       # keeps the bytes alive
        self.device = data.device.index
        self._h = C.c_void_p()
        with _on(self.device, stream):
            _check(_L.rrx_corpus_create_ex(self.device, _ptr(data), data.numel(),
                                           stripe, _stream_ptr(stream), C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None) and _L is not None:      # (_L is None during interpreter shutdown)
            _L.rrx_corpus_free(self._h)
            self._h = None

    @property
    def num_lines(self):
        return _L.rrx_corpus_num_lines(self._h)

    @property
    def num_bytes(self):
        return _L.rrx_corpus_num_bytes(self._h)

    @property
    def stripe(self):
        return _L.rrx_corpus_stripe_bytes(self._h)

    @property
    def one_launch(self):
        """True if the stride-2 table kernel needs no cleared bitmap on this corpus (rrx_corpus_one_launch): no bitmap word
        lies in the line ranges of three workgroups."""
        return bool(_L.rrx_corpus_one_launch(self._h, None))

    @property
    def one_launch_span(self):
        """The longest run of bitmap words of one workgroup behind its first (0 where one_launch is False)."""
        span = C.c_uint32(0)
        _L.rrx_corpus_one_launch(self._h, C.byref(span))
        return span.value

    def filter_lines(self, bits, invert=False, keep_newline=True, stream=None):
        """The lines a result bitmap selects - what `grep` prints - as a new column written on the device (rrx_bitmap_rank,
        rrx_filter_corpus_sizes, a torch.cumsum, rrx_pieces_fill): line i is selected iff bit i & 31 of bits[i >> 5] is 1 (invert: 0,
        grep -v); `bits` is what match_corpus_bits and contains_corpus_bits return, or any bitmap in that layout.  -> (rows
        int64[nsel], out_off int64[nsel + 1], out uint8): rows[k] is the number of the k-th selected line and out[out_off[k] :
        out_off[k + 1]] its bytes - with its '\n' where keep_newline is set and the text has it: `out` is then a corpus again.  No
        offsets array of the corpus is built.  Waits for the number of rows and for the output's size."""
        n = self.num_lines
        with _on(self.device, stream):
            s = _stream_ptr(stream)
            rank, nsel = _filter_rank(bits, n, invert, self.device, s)
            return _filter_column(self.data, nsel, lambda rows, length, src: _L.rrx_filter_corpus_sizes(self._h, _ptr(bits), int(bool(invert)), int(bool(keep_newline)),
                                                                                                        _ptr(rank), rows, length, src, s), self.device, s)


class Items:
    """A device-resident batch of explicit items - one byte buffer and an offsets array, item i = data[offsets[i] :
    offsets[i + 1] - trim] - indexed once (rrx_items) and matched by many patterns: RRegex.match_items."""

    def __init__(self, data, offsets, trim=0, stream=None):
        import torch
        assert data.is_cuda and data.dtype == torch.uint8 and data.is_contiguous()
        assert offsets.is_cuda and offsets.dtype in (torch.int64, torch.uint64) and offsets.is_contiguous() and offsets.numel() >= 1
        self.data, self.offsets, self.trim = data, offsets, trim       # kept alive: the handle points into them
        self.device = data.device.index
        self._h = C.c_void_p()
        with _on(self.device, stream):
            _check(_L.rrx_items_create(self.device, _ptr(data), C.c_void_p(offsets.data_ptr()),
                                       offsets.numel() - 1, trim, _stream_ptr(stream), C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None) and _L is not None:
            _L.rrx_items_free(self._h)
            self._h = None

    @property
    def num_items(self):
        return _L.rrx_items_count(self._h)

    @property
    def stripe_wise(self):
        """True if the batch admits the stripe-wise kernel (else every match runs lane per item)."""
        return bool(_L.rrx_items_stripe_wise(self._h))


class RRegex:
    """regex.h:212-228.  RRegex(pattern) compiles on the host (Parser.cpp:161-170)."""

    def __init__(self, pattern, engine=ENGINE_AUTO, device=0):
        if isinstance(pattern, str):
            pattern = pattern.encode("latin-1")
        self.pattern = pattern
        self.device = device
        self._h = C.c_void_p()
        _check(_L.rrx_compile_ex(pattern, engine, C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None) and _L is not None:
            _L.rrx_free(self._h)
            self._h = None

    # ---- the reference's interface for this path
    def get_acceptance_iter(self, text):
        if isinstance(text, str):
            text = text.encode("latin-1")
        return IteratorWrapper(self, text, self.device)

    # ---- batch entry
    def match_corpus_bits(self, corpus, out=None, stream=None):
        """THE HOT PATH (rrx_match_corpus): the accept bitmap as an int32 tensor, bit (i & 31) of word i >> 5 =
        line i accepted.  Asynchronous on `stream`."""
        import torch
        nw = _L.rrx_corpus_bitmap_words(corpus._h)
        with _on(corpus.device, stream):
            out = _out(out, nw, torch.int32, corpus.data.device)
            _check(_L.rrx_match_corpus(self._h, corpus._h, _ptr(out), _stream_ptr(stream)))
        return out

    def match_device_bits(self, data, cap_lines=None, out=None, stream=None):
        """One-shot (rrx_match_device): a device tensor nobody has indexed -> (accept bitmap as int32 words, number of
        strings).  With the stride-2 table engine the text is read once.  cap_lines bounds the number of strings the
        bitmap can hold (default: one per byte, the most a buffer can hold)."""
        import torch
        assert data.is_cuda and data.dtype == torch.uint8 and data.is_contiguous()
        n = data.numel()
        if cap_lines is None:
            cap_lines = n + 1
        cap_words = (cap_lines + 31) // 32
        with _on(data.device.index, stream):
            out = _out(out, cap_words, torch.int32, data.device)
            nlines = C.c_size_t(0)
            _check(_L.rrx_match_device(self._h, data.device.index, _ptr(data), n,
                                       C.c_void_p(out.data_ptr()), cap_words, C.byref(nlines), _stream_ptr(stream)))
        return out[:(nlines.value + 31) // 32], nlines.value

    def match_corpus(self, corpus, out=None, stream=None):
        """accept[i] = 1 iff line i of the corpus is accepted (one byte per line: bitmap + expansion)."""
        with _on(corpus.device, stream):
            return _bits_to_bytes(self.match_corpus_bits(corpus, stream=stream), corpus.num_lines, out, corpus.data.device, stream)

    def contains_corpus_bits(self, corpus, out=None, stream=None):
        """Which lines CONTAIN a match (rrx_contains_corpus): a bitmap of 32-bit words, an int32 tensor like match_corpus_bits',
        bit (i & 31) of word i >> 5 = some substring of line i is accepted, i.e. search_corpus would report a match for it.  NUL
        and bytes >= 0x80 are ordinary text here.  Asynchronous on `stream`."""
        import torch
        nw = _L.rrx_corpus_bitmap_words(corpus._h)
        with _on(corpus.device, stream):
            out = _out(out, nw, torch.int32, corpus.data.device)
            _check(_L.rrx_contains_corpus(self._h, corpus._h, _ptr(out), _stream_ptr(stream)))
        return out

    def contains_corpus(self, corpus, out=None, stream=None):
        """contains[i] = 1 iff line i of the corpus contains a match (one byte per line: bitmap + expansion)."""
        with _on(corpus.device, stream):
            return _bits_to_bytes(self.contains_corpus_bits(corpus, stream=stream), corpus.num_lines, out, corpus.data.device, stream)

    def search_corpus(self, corpus, stream=None):
        """Per string the accepted substring [start, end) with the smallest end, then the smallest start, as two int32
        tensors of offsets relative to the start of the string; (-1, -1) where nothing is accepted."""
        with _on(corpus.device, stream):
            start, end = _span_pair(corpus.num_lines, corpus.data.device)
            _check(_L.rrx_search_corpus(self._h, corpus._h, _ptr(start), _ptr(end), _stream_ptr(stream)))
        return start, end

    def search_longest_corpus(self, corpus, stream=None):
        """Per string the LEFTMOST-LONGEST match [start, end) (rrx_search_longest_corpus): the smallest start, then the largest end
        from there, as two int32 tensors of offsets relative to the start of the string; (-1, -1) where nothing is accepted.  Exactly
        what search_longest_extents gives for the strings as items; '\\n' never takes part in a match."""
        with _on(corpus.device, stream):
            n = corpus.num_lines                   # (a word at least: the entry refuses a null array, and reports an unsupported regex for no line too)
            start, end = _span_pair(max(n, 1), corpus.data.device)
            _check(_L.rrx_search_longest_corpus(self._h, corpus._h, _ptr(start), _ptr(end), _stream_ptr(stream)))
        return start[:n], end[:n]

    def search_all(self, corpus, stream=None):
        """ALL lazy matches of every string, left to right -> (count[n] int32, first[n] int64, start[total] int32,
        end[total] int32): the matches of string i are start/end[first[i] : first[i] + count[i]], relative to the string."""
        with _on(corpus.device, stream):
            s = _stream_ptr(stream)
            return _search_all_two_pass(corpus.data.device, corpus.num_lines,
                                        lambda c: _L.rrx_search_all_count(self._h, corpus._h, c, s),
                                        lambda f, st, en: _L.rrx_search_all_fill(self._h, corpus._h, f, st, en, s))

    def search_all_fused(self, corpus, cap=None, stream=None):
        """The same result through the one-call entry (rrx_search_all: one pass over the text) ->
        (first[n + 1] int64 CSR offsets, start[total] int32, end[total] int32).  cap: entries to provide for at first
        (default: two per string); the call is repeated with the exact size if there are more."""
        with _on(corpus.device, stream):
            s = _stream_ptr(stream)
            return _search_all_one_call(corpus.data.device, corpus.num_lines, cap,
                                        lambda f, st, en, cp, tot: _L.rrx_search_all(self._h, corpus._h, f, st, en, cp, tot, s))

    def match_items(self, items, out=None, stream=None):
        """One byte per item of an indexed batch (Items)."""
        import torch
        n = items.num_items
        with _on(items.device, stream):
            out = _out(out, n, torch.uint8, items.data.device)
            _check(_L.rrx_match_items(self._h, items._h, _ptr(out), _stream_ptr(stream)))
        return out

    def match_extents(self, data, offsets, trim=0, out=None, stream=None):
        """item i = data[offsets[i] : offsets[i+1] - trim]; '\\n' is an ordinary character."""
        import torch
        n, d, b, o = _batch(data, offsets)
        with _on(d, stream):
            out = _out(out, n, torch.uint8, data.device)
            _check(_L.rrx_match_extents(self._h, d, b, o, n, trim, _ptr(out), _stream_ptr(stream)))
        return out

    def contains_items_bits(self, items, out=None, stream=None):
        """Which items of an indexed batch (Items) CONTAIN a match (rrx_contains_items): a bitmap of 32-bit words, an int32 tensor,
        bit (i & 31) of word i >> 5 = some substring of item i is accepted.  '\\n', NUL and bytes >= 0x80 are ordinary text inside an
        item.  The bits of the last word beyond the last item are 0.  Asynchronous on `stream`."""
        import torch
        n = items.num_items
        nw = (n + 31) // 32
        with _on(items.device, stream):
            out = _out(out, nw, torch.int32, items.data.device)
            _check(_L.rrx_contains_items(self._h, items._h, _ptr(out), _stream_ptr(stream)))
        return out

    def contains_items(self, items, out=None, stream=None):
        """contains[i] = 1 iff item i of the indexed batch contains a match (one byte per item: bitmap + expansion)."""
        with _on(items.device, stream):
            return _bits_to_bytes(self.contains_items_bits(items, stream=stream), items.num_items, out, items.data.device, stream)

    def contains_extents_bits(self, data, offsets, trim=0, out=None, stream=None):
        """The same for a batch nobody has indexed (rrx_contains_extents): item i = data[offsets[i] : offsets[i+1] - trim] -> the
        bitmap of the items that contain a match, ceil(n / 32) int32 words."""
        import torch
        n, d, b, o = _batch(data, offsets)
        nw = (n + 31) // 32
        with _on(d, stream):
            out = _out(out, nw, torch.int32, data.device)
            _check(_L.rrx_contains_extents(self._h, d, b, o, n, trim, _ptr(out), _stream_ptr(stream)))
        return out

    def contains_extents(self, data, offsets, trim=0, out=None, stream=None):
        """contains[i] = 1 iff item i = data[offsets[i] : offsets[i+1] - trim] contains a match (one byte per item)."""
        n, d = _batch(data, offsets)[:2]
        with _on(d, stream):
            return _bits_to_bytes(self.contains_extents_bits(data, offsets, trim=trim, stream=stream), n, out, data.device, stream)

    def search_items(self, items, stream=None):
        """Per item of an indexed batch (Items) the accepted substring [start, end) with the smallest end, then the smallest start
        (rrx_search_items), as two int32 tensors of offsets relative to the start of the item; (-1, -1) where nothing is accepted.
        '\\n', NUL and bytes >= 0x80 are ordinary text inside an item.  Asynchronous on `stream`."""
        with _on(items.device, stream):
            start, end = _span_pair(items.num_items, items.data.device)
            _check(_L.rrx_search_items(self._h, items._h, _ptr(start), _ptr(end), _stream_ptr(stream)))
        return start, end

    def search_extents(self, data, offsets, trim=0, stream=None):
        """The same for a batch nobody has indexed (rrx_search_extents): item i = data[offsets[i] : offsets[i+1] - trim] ->
        (start, end), int32, (-1, -1) where nothing is accepted.  Nothing is read back: the call can be captured into a graph."""
        n, d, b, o = _batch(data, offsets)
        with _on(d, stream):
            start, end = _span_pair(n, data.device)
            _check(_L.rrx_search_extents(self._h, d, b, o, n, trim, _ptr(start), _ptr(end), _stream_ptr(stream)))
        return start, end

    def search_all_items(self, items, stream=None):
        """ALL matches of every item of an indexed batch (Items), left to right (rrx_search_all_items_count / _fill) ->
        (count[n] int32, first[n] int64, start[total] int32, end[total] int32), shaped as search_all returns them: the matches of
        item i are start/end[first[i] : first[i] + count[i]], relative to the item.  Match k + 1 is searched in the rest of the item
        behind match k; '\\n', NUL and bytes >= 0x80 are ordinary text inside an item."""
        with _on(items.device, stream):
            s = _stream_ptr(stream)
            return _search_all_two_pass(items.data.device, items.num_items,
                                        lambda c: _L.rrx_search_all_items_count(self._h, items._h, c, s),
                                        lambda f, st, en: _L.rrx_search_all_items_fill(self._h, items._h, f, st, en, s))

    def search_all_extents(self, data, offsets, trim=0, stream=None):
        """The same for a batch nobody has indexed (rrx_search_all_extents_count / _fill): item i = data[offsets[i] : offsets[i+1] - trim]."""
        n, d, b, o = _batch(data, offsets)
        with _on(d, stream):
            s = _stream_ptr(stream)
            return _search_all_two_pass(data.device, n,
                                        lambda c: _L.rrx_search_all_extents_count(self._h, d, b, o, n, trim, c, s),
                                        lambda f, st, en: _L.rrx_search_all_extents_fill(self._h, d, b, o, n, trim, f, st, en, s))

    def search_all_items_fused(self, items, cap=None, stream=None):
        """The same result through the one-call entry (rrx_search_all_items) -> (first[n + 1] int64 CSR offsets, start[total] int32,
        end[total] int32).  cap: entries to provide for at first (default: two per item); the call is repeated with the exact size
        if there are more."""
        with _on(items.device, stream):
            s = _stream_ptr(stream)
            return _search_all_one_call(items.data.device, items.num_items, cap,
                                        lambda f, st, en, cp, tot: _L.rrx_search_all_items(self._h, items._h, f, st, en, cp, tot, s))

    def search_all_extents_fused(self, data, offsets, trim=0, cap=None, stream=None):
        """The one-call entry for a batch nobody has indexed (rrx_search_all_extents) -> (first[n + 1], start, end)."""
        n, d, b, o = _batch(data, offsets)
        with _on(d, stream):
            s = _stream_ptr(stream)
            return _search_all_one_call(data.device, n, cap,
                                        lambda f, st, en, cp, tot: _L.rrx_search_all_extents(self._h, d, b, o, n, trim, f, st, en, cp, tot, s))

    def search_longest_items(self, items, stream=None):
        """Per item of an indexed batch (Items) the LEFTMOST-LONGEST match [start, end) (rrx_search_longest_items): the smallest start
        of any accepted substring, then the largest end from there, as two int32 tensors of offsets relative to the start of the item;
        (-1, -1) where nothing is accepted.  '\\n', NUL and bytes >= 0x80 are ordinary text inside an item.  Asynchronous on `stream`."""
        with _on(items.device, stream):
            start, end = _span_pair(items.num_items, items.data.device)
            _check(_L.rrx_search_longest_items(self._h, items._h, _ptr(start), _ptr(end), _stream_ptr(stream)))
        return start, end

    def search_longest_extents(self, data, offsets, trim=0, stream=None):
        """The same for a batch nobody has indexed (rrx_search_longest_extents): item i = data[offsets[i] : offsets[i+1] - trim] ->
        (start, end), int32, (-1, -1) where nothing is accepted.  Nothing is read back: the call can be captured into a graph."""
        n, d, b, o = _batch(data, offsets)
        with _on(d, stream):
            start, end = _span_pair(n, data.device)
            _check(_L.rrx_search_longest_extents(self._h, d, b, o, n, trim, _ptr(start), _ptr(end), _stream_ptr(stream)))
        return start, end

    @staticmethod
    def _search_all_longest_marks(data, n):
        """The marks buffer of the two-pass leftmost-longest entries for a batch of n items inside `data`: int32, sized from
        data.numel() (rrx_search_all_longest_marks_words), uninitialised - the count pass stores every word that the fill pass reads."""
        import torch
        words = _L.rrx_search_all_longest_marks_words(data.numel(), n)
        return torch.empty(words, dtype=torch.int32, device=data.device), words

    def search_all_longest_items(self, items, stream=None):
        """ALL LEFTMOST-LONGEST matches of every item of an indexed batch (Items), left to right (rrx_search_all_longest_items_count /
        _fill) -> (count[n] int32, first[n] int64, start[total] int32, end[total] int32), shaped as search_all_items returns them.
        Match k + 1 is the leftmost-longest match of the rest of the item behind match k (one byte further after an empty match):
        [0-9]+ on b"a1 22 333" gives [1,2) [3,5) [6,9).  '\\n', NUL and bytes >= 0x80 are ordinary text inside an item."""
        with _on(items.device, stream):
            s = _stream_ptr(stream)
            marks, words = self._search_all_longest_marks(items.data, items.num_items)
            m = C.c_void_p(marks.data_ptr())
            return _search_all_two_pass(items.data.device, items.num_items,
                                        lambda c: _L.rrx_search_all_longest_items_count(self._h, items._h, m, words, c, s),
                                        lambda f, st, en: _L.rrx_search_all_longest_items_fill(self._h, items._h, m, words, f, st, en, s))

    def search_all_longest_extents(self, data, offsets, trim=0, stream=None):
        """The same for a batch nobody has indexed (rrx_search_all_longest_extents_count / _fill): item i = data[offsets[i] : offsets[i+1] - trim]."""
        n, d, b, o = _batch(data, offsets)
        with _on(d, stream):
            s = _stream_ptr(stream)
            marks, words = self._search_all_longest_marks(data, n)
            m = C.c_void_p(marks.data_ptr())
            return _search_all_two_pass(data.device, n,
                                        lambda c: _L.rrx_search_all_longest_extents_count(self._h, d, b, o, n, trim, m, words, c, s),
                                        lambda f, st, en: _L.rrx_search_all_longest_extents_fill(self._h, d, b, o, n, trim, m, words, f, st, en, s))

    def search_all_longest_items_fused(self, items, cap=None, stream=None):
        """The same result through the one-call entry (rrx_search_all_longest_items) -> (first[n + 1] int64 CSR offsets, start[total]
        int32, end[total] int32).  cap: entries to provide for at first (default: two per item); the call is repeated with the exact
        size if there are more."""
        with _on(items.device, stream):
            s = _stream_ptr(stream)
            return _search_all_one_call(items.data.device, items.num_items, cap,
                                        lambda f, st, en, cp, tot: _L.rrx_search_all_longest_items(self._h, items._h, f, st, en, cp, tot, s))

    def search_all_longest_extents_fused(self, data, offsets, trim=0, cap=None, stream=None):
        """The one-call entry for a batch nobody has indexed (rrx_search_all_longest_extents) -> (first[n + 1], start, end)."""
        n, d, b, o = _batch(data, offsets)
        with _on(d, stream):
            s = _stream_ptr(stream)
            return _search_all_one_call(data.device, n, cap,
                                        lambda f, st, en, cp, tot: _L.rrx_search_all_longest_extents(self._h, d, b, o, n, trim, f, st, en, cp, tot, s))

    def replace_all_longest_extents(self, data, offsets, repl, trim=0, cap=None, stream=None):
        """regexp_replace on a string column (rrx_replace_all_longest_extents): item i = data[offsets[i] : offsets[i+1] - trim] with
        EVERY LEFTMOST-LONGEST match replaced by the literal `repl` (bytes; group references: replace_groups_longest_extents) -> (out uint8, out_off int64[n + 1]),
        output item i = out[out_off[i] : out_off[i + 1]] - re.sub(p, lambda m: repl, item); the separators are not copied.  cap: bytes
        to provide for at first (default: the size of `data`); the call is repeated with the exact size if the column is larger."""
        assert isinstance(repl, (bytes, bytearray))
        (n, d, b, o), rep = _batch(data, offsets), bytes(repl)
        with _on(d, stream):
            s = _stream_ptr(stream)
            return _replace_one_call(data.device, n, int(cap) if cap is not None else data.numel(),
                                     lambda f, out, cp, tot: _L.rrx_replace_all_longest_extents(self._h, d, b, o, n, trim, rep, len(rep), f, out, cp, tot, s))

    def replace_all_longest_items(self, items, repl, cap=None, stream=None):
        """The same for an indexed batch (rrx_replace_all_longest_items) -> (out uint8, out_off int64[n + 1])."""
        assert isinstance(repl, (bytes, bytearray))
        rep = bytes(repl)
        with _on(items.device, stream):
            s = _stream_ptr(stream)
            return _replace_one_call(items.data.device, items.num_items, int(cap) if cap is not None else items.data.numel(),
                                     lambda f, out, cp, tot: _L.rrx_replace_all_longest_items(self._h, items._h, rep, len(rep), f, out, cp, tot, s))

    def extract_all_longest_extents(self, data, offsets, trim=0, cap=None, pieces_cap=None, stream=None):
        """regexp_extract_all on a string column (rrx_extract_all_longest_extents): EVERY LEFTMOST-LONGEST match of item i =
        data[offsets[i] : offsets[i+1] - trim] as a list<binary> column -> (out uint8, piece_off int64[npieces + 1], list_off
        int64[n + 1]): the matches of item i are the pieces list_off[i] .. list_off[i + 1], piece p = out[piece_off[p] :
        piece_off[p + 1]] - [x.group() for x in re.finditer(p, item)].  cap / pieces_cap: bytes and pieces to provide for at first
        (default: the size of `data`, two per item); the call is repeated with the exact sizes if the column is larger."""
        n, d, b, o = _batch(data, offsets)
        with _on(d, stream):
            s = _stream_ptr(stream)
            return _pieces_one_call(data.device, n, data.numel(), cap, pieces_cap, lambda lo, po, pc, out, cp, npc, tot:
                                    _L.rrx_extract_all_longest_extents(self._h, d, b, o, n, trim, lo, po, pc, out, cp, npc, tot, s))

    def extract_all_longest_items(self, items, cap=None, pieces_cap=None, stream=None):
        """The same for an indexed batch (rrx_extract_all_longest_items)."""
        with _on(items.device, stream):
            s = _stream_ptr(stream)
            return _pieces_one_call(items.data.device, items.num_items, items.data.numel(), cap, pieces_cap, lambda lo, po, pc, out, cp, npc, tot:
                                    _L.rrx_extract_all_longest_items(self._h, items._h, lo, po, pc, out, cp, npc, tot, s))

    def split_longest_extents(self, data, offsets, trim=0, cap=None, pieces_cap=None, stream=None):
        """split on a string column (rrx_split_longest_extents): what lies between the leftmost-longest matches of every item, one
        piece more than it has matches, in the shape extract_all_longest_extents returns - re.split(p, item) for a pattern without
        groups; the separators (`trim`) are not copied."""
        n, d, b, o = _batch(data, offsets)
        with _on(d, stream):
            s = _stream_ptr(stream)
            return _pieces_one_call(data.device, n, data.numel(), cap, pieces_cap, lambda lo, po, pc, out, cp, npc, tot:
                                    _L.rrx_split_longest_extents(self._h, d, b, o, n, trim, lo, po, pc, out, cp, npc, tot, s))

    def split_longest_items(self, items, cap=None, pieces_cap=None, stream=None):
        """The same for an indexed batch (rrx_split_longest_items)."""
        with _on(items.device, stream):
            s = _stream_ptr(stream)
            return _pieces_one_call(items.data.device, items.num_items, items.data.numel(), cap, pieces_cap, lambda lo, po, pc, out, cp, npc, tot:
                                    _L.rrx_split_longest_items(self._h, items._h, lo, po, pc, out, cp, npc, tot, s))

    def filter_contains_extents(self, data, offsets, trim=0, invert=False, cap=None, rows_cap=None, stream=None):
        """SELECT col WHERE col RLIKE p on a string column (rrx_filter_contains_extents): the items data[offsets[i] : offsets[i+1] -
        trim] that CONTAIN a match (invert: that do not) as a new column -> (rows int64[nrows], out_off int64[nrows + 1], out uint8):
        rows[k] is the number of the k-th surviving item, out[out_off[k] : out_off[k + 1]] its bytes; the separators are not copied.
        cap / rows_cap: bytes and rows to provide for at first (default: the size of `data`, every item); the call is repeated with
        the exact sizes if the column is larger."""
        n, d, b, o = _batch(data, offsets)
        with _on(d, stream):
            s = _stream_ptr(stream)
            return _filter_one_call(data.device, n, data.numel(), cap, rows_cap, lambda rows, oo, rc, out, cp, nr, tot:
                                    _L.rrx_filter_contains_extents(self._h, d, b, o, n, trim, int(bool(invert)), rows, oo, rc, out, cp, nr, tot, s))

    def filter_contains_items(self, items, invert=False, cap=None, rows_cap=None, stream=None):
        """The same for an indexed batch (rrx_filter_contains_items: contains runs stripe-wise where the batch admits it)."""
        with _on(items.device, stream):
            s = _stream_ptr(stream)
            return _filter_one_call(items.data.device, items.num_items, items.data.numel(), cap, rows_cap, lambda rows, oo, rc, out, cp, nr, tot:
                                    _L.rrx_filter_contains_items(self._h, items._h, int(bool(invert)), rows, oo, rc, out, cp, nr, tot, s))

    def filter_contains_corpus(self, corpus, invert=False, keep_newline=True, cap=None, rows_cap=None, stream=None):
        """grep (invert: grep -v) on a '\n'-corpus (rrx_filter_contains_corpus): the lines that contain a match, in the shape
        filter_contains_extents returns - with their '\n' where keep_newline is set and the text has it, so that `out` is a corpus
        again and `grep p1 | grep p2` needs no host step."""
        with _on(corpus.device, stream):
            s = _stream_ptr(stream)
            return _filter_one_call(corpus.data.device, corpus.num_lines, corpus.num_bytes, cap, rows_cap, lambda rows, oo, rc, out, cp, nr, tot:
                                    _L.rrx_filter_contains_corpus(self._h, corpus._h, int(bool(invert)), int(bool(keep_newline)), rows, oo, rc, out, cp, nr,
                                                                  tot, s))

    def match_string(self, data, stream=None):
        """ONE device-resident string of any length (regex.h:156-159); '\n' is an ordinary character.  -> bool"""
        import torch
        assert data.is_cuda and data.dtype == torch.uint8
        with _on(data.device.index, stream):
            out = torch.zeros(1, dtype=torch.uint8, device=data.device)
            _check(_L.rrx_match_string(self._h, data.device.index, _ptr(data), data.numel(),
                                       C.c_void_p(out.data_ptr()), _stream_ptr(stream)))
        return bool(out.item())

    def search_longest_string(self, data, stream=None):
        """The LEFTMOST-LONGEST match inside ONE device-resident string of any length (rrx_search_longest_string): what
        search_longest_extents gives for the whole string as one item, without its 32-bit cap; '\n' is an ordinary character.
        -> (start, end) as ints, (-1, -1) for none"""
        import torch
        assert data.is_cuda and data.dtype == torch.uint8
        with _on(data.device.index, stream):
            out = torch.zeros(2, dtype=torch.int64, device=data.device)
            _check(_L.rrx_search_longest_string(self._h, data.device.index, _ptr(data), data.numel(), _ptr(out), _stream_ptr(stream)))
        start, end = out.tolist()
        return start, end

    def contains_string(self, data, stream=None):
        """Whether ONE device-resident string of any length contains a match (rrx_contains_string).  -> bool"""
        import torch
        assert data.is_cuda and data.dtype == torch.uint8
        with _on(data.device.index, stream):
            out = torch.zeros(1, dtype=torch.uint8, device=data.device)
            _check(_L.rrx_contains_string(self._h, data.device.index, _ptr(data), data.numel(), _ptr(out), _stream_ptr(stream)))
        return bool(out.item())

    def match_host(self, data):
        """Host bytes in, numpy accept vector out (upload + index + match + download; synchronous)."""
        import numpy as np
        a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
        cap = len(a) + 1                       # a buffer of n bytes holds at most n + 1 strings; untouched pages are free
        out = np.empty(cap, dtype=np.uint8)
        n = C.c_size_t(0)
        _check(_L.rrx_match_host(self._h, self.device, C.c_void_p(a.ctypes.data if len(a) else 0), len(a),
                                 C.c_void_p(out.ctypes.data), cap, C.byref(n)))
        return out[:n.value]

    # ---- introspection (parity checks on the construction; see include/rrx.h)
    @property
    def states_n(self):
        return _L.rrx_num_states(self._h)

    @property
    def set_class(self):
        return _L.rrx_set_class(self._h)

    @property
    def initial(self):
        return _L.rrx_ref_initial(self._h)

    def finals(self):
        return [s for s in range(self.states_n) if _L.rrx_ref_is_final(self._h, s)]

    def row(self, state, c):
        n = self.states_n
        buf = (C.c_uint32 * max(n, 1))()
        k = _L.rrx_ref_row(self._h, state, c, buf, n)
        return list(buf[:k])

    @property
    def engine(self):
        return _L.rrx_engine(self._h)

    @property
    def engine_name(self):
        return _L.rrx_engine_name(self._h).decode()

    @property
    def contains_engine_name(self):
        """The table form contains_corpus runs on (host only); raises RRegexError where the pattern has no contains table."""
        name = _L.rrx_contains_engine_name(self._h)
        if name is None:
            raise RRegexError(_L.rrx_last_error().decode("latin-1"))
        return name.decode()

    @property
    def contains_states(self):
        """States of the contains table, the SKIP row included; 0 where the pattern has none (host only)."""
        return _L.rrx_contains_states(self._h)

    @property
    def useful_states(self):
        return _L.rrx_useful_states(self._h)

    def order_table(self, sample, lanes, bytes_per_lane):
        """Order the stride-2 table by a text sample of the caller's (numpy uint8, lanes x bytes_per_lane, lane-major) before
        the first match (rrx_order_table).  Host only."""
        import numpy as np
        a = np.ascontiguousarray(sample, dtype=np.uint8)
        assert a.size >= lanes * bytes_per_lane
        _check(_L.rrx_order_table(self._h, C.c_void_p(a.ctypes.data), lanes, bytes_per_lane))
        return self.table_order

    def set_background_order(self, enabled):
        """rrx_set_option(RRX_OPT_BACKGROUND_ORDER): False forbids the library's own thread and device allocations for the profiled
        table order (the table stays as numbered unless order_table is called)."""
        _check(_L.rrx_set_option(self._h, OPT_BACKGROUND_ORDER, 1 if enabled else 0))

    def learn_table(self, text):
        """rrx_learn_table: build the sampled table (an automaton AUTO leaves on the NFA lane engine) from a text sample - bytes or a
        numpy uint8 array of whole lines.  Returns (table states, open transitions)."""
        import numpy as np
        a = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else np.ascontiguousarray(text, dtype=np.uint8)
        _check(_L.rrx_learn_table(self._h, C.c_void_p(a.ctypes.data), a.size))
        return self.sampled_table

    def set_sampled_table(self, enabled):
        _check(_L.rrx_set_option(self._h, OPT_SAMPLED_TABLE, 1 if enabled else 0))

    @property
    def sampled_table(self):
        """None, or (table states, open transitions) of the sampled table in use."""
        n, o = C.c_uint32(0), C.c_uint32(0)
        return (n.value, o.value) if _L.rrx_sampled_table(self._h, C.byref(n), C.byref(o)) == 1 else None

    def sampled_escapes(self):
        """Lines the NFA engine had to decide in the last sampled-table launch on this regex' device (waits for the device)."""
        n = C.c_uint64(0)
        _check(_L.rrx_sampled_escapes(self._h, self.device, C.byref(n)))
        return n.value

    @property
    def sampled_table_pending(self):
        return _L.rrx_sampled_table(self._h, None, None) == 2

    @property
    def sampled_table_retired(self):
        """A corpus escaped from the sampled table (more than 5 % of its lines): the regex is back on the NFA engine."""
        return _L.rrx_sampled_table(self._h, None, None) == 3

    def set_flush_slots(self, slots):
        """rrx_set_option(RRX_OPT_FLUSH_SLOTS): 0 = automatic, or 1 ... 32 slots between two common flushes of the stride-2 kernel."""
        _check(_L.rrx_set_option(self._h, OPT_FLUSH_SLOTS, int(slots)))

    def flush_slots(self, corpus):
        """(slots, compiled_in): the stride-2 kernel's common flush period for this regex on `corpus`, and whether it is the
        kernel with the period compiled in (rrx_match_flush_slots)."""
        fixed = C.c_int(0)
        slots = _L.rrx_match_flush_slots(self._h, corpus._h, C.byref(fixed))
        return slots, bool(fixed.value)

    def set_search_anchored(self, enabled):
        """rrx_set_option(RRX_OPT_SEARCH_ANCHORED): False builds the search kernels' forward table without the product that tells
        the matches starting at the line start (fewer rows; every match start is walked back to).  Before the first search."""
        _check(_L.rrx_set_option(self._h, OPT_SEARCH_ANCHORED, 1 if enabled else 0))

    def set_items_stride2(self, enabled):
        """rrx_set_option(RRX_OPT_ITEMS_STRIDE2): False keeps large batches of explicit items with separators (trim 1) on the
        byte-stride items kernel instead of the stride-2 table of their own."""
        _check(_L.rrx_set_option(self._h, OPT_ITEMS_STRIDE2, 1 if enabled else 0))

    def set_contains_nfa(self, mode):
        """rrx_set_option(RRX_OPT_CONTAINS_NFA): 0 keeps the three contains entries on the contains table (a pattern without one
        raises), 1 runs them on the shift-and NFA lane engine where the pattern has no table, 2 always (tests, A/B measurements).
        Same results; the NFA route is bound by the VALU, in another speed class than the tables.  Any other value raises."""
        _check(_L.rrx_set_option(self._h, OPT_CONTAINS_NFA, int(mode)))

    def set_units_per_workgroup(self, units):
        """rrx_set_option(RRX_OPT_UNITS_PER_WORKGROUP): accepted and ignored - the kernel that handed its stripes out in units
        inside the workgroup is gone (it never won); the value is still checked (0 ... 65536)."""
        _check(_L.rrx_set_option(self._h, OPT_UNITS_PER_WORKGROUP, int(units)))

    @property
    def table_order(self):
        """None, or (before, after): the stride-2 table is laid out in an order profiled on the first large corpus this regex
        met; the mean number of distinct entries in the fullest LDS bank per half-wave on the sample, as numbered / as ordered."""
        b, a = C.c_double(0), C.c_double(0)
        return (b.value, a.value) if _L.rrx_table_order(self._h, C.byref(b), C.byref(a)) == 1 else None

    @property
    def table_order_pending(self):
        """True while the background search for a profiled table order is running."""
        return _L.rrx_table_order(self._h, None, None) == 2

    @property
    def byte_classes(self):
        return _L.rrx_byte_classes(self._h)

    @property
    def words_per_set(self):
        return _L.rrx_words_per_set(self._h)

    def program(self, kind):
        """Serialised device program (numpy uint32), or None if that form was not built."""
        import numpy as np
        n = _L.rrx_program_words(self._h, kind, None, 0)
        if not n:
            return None
        out = np.zeros(n, dtype=np.uint32)
        _L.rrx_program_words(self._h, kind, C.c_void_p(out.ctypes.data), n)
        return out

    @property
    def accepts_empty(self):
        return bool(_L.rrx_accepts_empty(self._h))


class _BorrowedRRegex(RRegex):
    """An RRegex over a handle that somebody else owns (RGroup.regex): never freed here, the owner kept alive."""

    def __init__(self, handle, pattern, device, owner):
        self.pattern, self.device, self._h, self._owner = pattern, device, C.c_void_p(handle), owner

    def __del__(self):
        self._h = None


class RGroup:
    """regexp_extract with a capture group on a string column (rrx_group): the pattern is a concatenation A(B)C and `group` selects
    (B) - the unescaped '(' outside brackets are counted from 1, nested ones too; the selected one must be at the top level, not
    repeated, and the top level must hold no '|' (RRegexError otherwise).  For every item the group's span lies inside the item's
    LEFTMOST-LONGEST match [s, e): start = the largest i with A accepting item[s:i] and BC accepting item[i:e], end = the largest j
    with B accepting item[i:j] and C accepting item[j:e].  RGroup(b"https?://([^/]+)/.*", 1) on b"see http://example.com/a/b" gives
    [11, 22)."""

    def __init__(self, pattern, group, engine=ENGINE_AUTO, device=0):
        if isinstance(pattern, str):
            pattern = pattern.encode("latin-1")
        self.pattern, self.group, self.device = pattern, group, device
        self._h = C.c_void_p()
        _check(_L.rrx_group_compile_ex(pattern, group, engine, C.byref(self._h)))
        self.regex = _BorrowedRRegex(_L.rrx_group_regex(self._h), pattern, device, self)   # the whole pattern: search_longest_*, contains_* ...

    def __del__(self):
        if getattr(self, "_h", None) and _L is not None:
            if getattr(self, "regex", None) is not None:
                self.regex._h = None
            _L.rrx_group_free(self._h)
            self._h = None

    @property
    def parts(self):
        """The source text of (A, B, C) as bytes; an absent part is b""."""
        out = []
        for which in range(3):
            n = _L.rrx_group_part(self._h, which, None, 0)
            buf = C.create_string_buffer(max(n, 1))
            _L.rrx_group_part(self._h, which, buf, n)
            out.append(buf.raw[:n])
        return tuple(out)

    def program(self, which):
        """One of the four tables (PROGRAM_GROUP_A / _REV_BC / _B / _REV_C) in the DFA layout (numpy uint32), None for an absent part's."""
        import numpy as np
        n = _L.rrx_group_program_words(self._h, which, None, 0)
        if not n:
            return None
        out = np.zeros(n, dtype=np.uint32)
        _L.rrx_group_program_words(self._h, which, C.c_void_p(out.ctypes.data), n)
        return out

    @staticmethod
    def _marks(data, n):
        """The marks buffer of a batch of n items inside `data`, sized from data.numel() as the all-longest entries size theirs."""
        import torch
        words = _L.rrx_search_all_longest_marks_words(data.numel(), n)
        return torch.empty(words, dtype=torch.int32, device=data.device), words

    @staticmethod
    def _outputs(n, device, out):
        import torch
        if out is not None:
            assert all(t.is_cuda and t.dtype in (torch.int32, torch.uint32) and t.is_contiguous() and t.numel() >= n for t in out)
            return out
        return _span_pair(n, device)

    def spans_extents(self, data, offsets, match_start, match_end, trim=0, out=None, stream=None):
        """From a span list - (match_start, match_end) int32 per item, relative to the item, as RRegex.search_longest_extents returns
        it for self.regex - to the group's spans (rrx_group_spans_extents) -> (start, end) int32, (-1, -1) where the item has no match
        or the span is not one.  out: the two result tensors; they may be match_start / match_end themselves.  Asynchronous."""
        n, d, b, o = _batch(data, offsets)
        with _on(d, stream):
            start, end = self._outputs(n, data.device, out)
            marks, words = self._marks(data, n)
            _check(_L.rrx_group_spans_extents(self._h, d, b, o, n, trim, _ptr(match_start), _ptr(match_end), _ptr(marks), words, _ptr(start), _ptr(end),
                                              _stream_ptr(stream)))
        return start, end

    def spans_items(self, items, match_start, match_end, out=None, stream=None):
        """The same for an indexed batch (rrx_group_spans_items)."""
        n = items.num_items
        with _on(items.device, stream):
            start, end = self._outputs(n, items.data.device, out)
            marks, words = self._marks(items.data, n)
            _check(_L.rrx_group_spans_items(self._h, items._h, _ptr(match_start), _ptr(match_end), _ptr(marks), words, _ptr(start), _ptr(end),
                                            _stream_ptr(stream)))
        return start, end

    def spans_list_extents(self, data, offsets, first, match_start, match_end, trim=0, out=None, marks=None, stream=None):
        """spans_extents for every match of a match list (rrx_group_spans_list_extents): match k of item i is slot first[i] + k of
        match_start / match_end, as every search_all*_fused method returns them -> (start, end) int32 indexed by the slot, (-1, -1)
        where the slot has no split.  out: the two result tensors (at least first[-1] entries); they may be match_start / match_end
        themselves.  Asynchronous."""
        n, d, b, o = _batch(data, offsets)
        with _on(d, stream):
            start, end = self._outputs(match_start.numel(), data.device, out)
            if marks is None:
                marks = self._marks(data, n)[0]
            _check(_L.rrx_group_spans_list_extents(self._h, d, b, o, n, trim, _ptr(first), _ptr(match_start), _ptr(match_end), _ptr(marks), marks.numel(),
                                                   _ptr(start), _ptr(end), _stream_ptr(stream)))
        return start, end

    def spans_list_items(self, items, first, match_start, match_end, out=None, marks=None, stream=None):
        """The same for an indexed batch (rrx_group_spans_list_items)."""
        n = items.num_items
        with _on(items.device, stream):
            start, end = self._outputs(match_start.numel(), items.data.device, out)
            if marks is None:
                marks = self._marks(items.data, n)[0]
            _check(_L.rrx_group_spans_list_items(self._h, items._h, _ptr(first), _ptr(match_start), _ptr(match_end), _ptr(marks), marks.numel(), _ptr(start),
                                                 _ptr(end), _stream_ptr(stream)))
        return start, end

    def extract_extents(self, data, offsets, trim=0, out=None, marks=None, stream=None):
        """The group's span per item of a batch nobody has indexed, the search included (rrx_extract_group_longest_extents): item i =
        data[offsets[i] : offsets[i+1] - trim] -> (start, end) int32, (-1, -1) where nothing is accepted.  Nothing is read back: with
        `out` and `marks` (an int32 tensor of rrx_search_all_longest_marks_words words) given, the call can be captured into a graph."""
        n, d, b, o = _batch(data, offsets)
        with _on(d, stream):
            start, end = self._outputs(n, data.device, out)
            if marks is None:
                marks = self._marks(data, n)[0]
            _check(_L.rrx_extract_group_longest_extents(self._h, d, b, o, n, trim, _ptr(marks), marks.numel(), _ptr(start), _ptr(end), _stream_ptr(stream)))
        return start, end

    def extract_items(self, items, out=None, marks=None, stream=None):
        """The same for an indexed batch (rrx_extract_group_longest_items)."""
        n = items.num_items
        with _on(items.device, stream):
            start, end = self._outputs(n, items.data.device, out)
            if marks is None:
                marks = self._marks(items.data, n)[0]
            _check(_L.rrx_extract_group_longest_items(self._h, items._h, _ptr(marks), marks.numel(), _ptr(start), _ptr(end), _stream_ptr(stream)))
        return start, end

    def extract_column(self, data, offsets, trim=0, stream=None):
        """regexp_extract(col, pattern, group) as a column, written on the device -> (valid bool[n], out_offsets int64[n + 1], out_bytes
        uint8): output item i = out_bytes[out_offsets[i] : out_offsets[i + 1]] is the group's text; an item without a match is invalid
        and empty.  The spans (extract_extents), their lengths, a torch.cumsum, then rrx_pieces_fill.  Waits for the output's size."""
        import torch
        n = offsets.numel() - 1
        d = data.device.index
        with _on(d, stream):
            start, end = self.extract_extents(data, offsets, trim=trim, stream=stream)
            valid = start >= 0
            if not n:
                return valid, torch.zeros(1, dtype=torch.int64, device=data.device), torch.empty(0, dtype=torch.uint8, device=data.device)
            out_off, out = _offsets_and_bytes(torch.where(valid, end - start, torch.zeros_like(start)), data.device)
            src = (offsets[:n].to(torch.int64) + torch.where(valid, start, torch.zeros_like(start)).to(torch.int64)).contiguous()
            _check(_L.rrx_pieces_fill(d, _ptr(data), _ptr(src), _ptr(out_off), n, _ptr(out), _stream_ptr(stream)))
        return valid, out_off, out


def _group_handles(groups):
    """The handle array of the one-call forms: groups[g - 1] is the RGroup of group g, None where the template does not use it."""
    assert len(groups) and all(g is None or isinstance(g, RGroup) for g in groups)
    return (C.c_void_p * len(groups))(*[g._h if g is not None else None for g in groups])


def replace_groups_longest_extents(groups, template, data, offsets, trim=0, cap=None, stream=None):
    """regexp_replace with group references on a string column (rrx_replace_groups_longest_extents): item i = data[offsets[i] :
    offsets[i+1] - trim] with EVERY LEFTMOST-LONGEST match of the groups' pattern replaced by `template` (a Template, or bytes) ->
    (out uint8, out_off int64[n + 1]).  groups[g - 1] is the RGroup of group g of ONE pattern (None for a group the template does not
    reference); each group's span follows RGroup's rule on its own.  cap: bytes to provide for at first (default: the size of
    `data`); the call is repeated with the exact size if the column is larger."""
    tpl = template if isinstance(template, Template) else Template(template)
    h = _group_handles(groups)
    n, d, b, o = _batch(data, offsets)
    with _on(d, stream):
        s = _stream_ptr(stream)
        return _replace_one_call(data.device, n, int(cap) if cap is not None else data.numel(),
                                 lambda f, out, cp, tot: _L.rrx_replace_groups_longest_extents(h, len(groups), tpl._h, d, b, o, n, trim, f, out, cp, tot, s))


def replace_groups_longest_items(groups, template, items, cap=None, stream=None):
    """The same for an indexed batch (rrx_replace_groups_longest_items) -> (out uint8, out_off int64[n + 1])."""
    tpl = template if isinstance(template, Template) else Template(template)
    h = _group_handles(groups)
    with _on(items.device, stream):
        s = _stream_ptr(stream)
        return _replace_one_call(items.data.device, items.num_items, int(cap) if cap is not None else items.data.numel(),
                                 lambda f, out, cp, tot: _L.rrx_replace_groups_longest_items(h, len(groups), tpl._h, items._h, f, out, cp, tot, s))


class RMulti:
    """A set of 1 to 32 patterns on a string column (rrx_multi): which of them does each item contain, in one walk over the column.
    Bit k of an item's mask is set exactly when RRegex(patterns[k]).contains_extents says 1 for that item.  The members are cut
    into groups that share one product table each (greedy in set order: `max_rows` rows per table at most, 0 = 65535, and 64 KiB
    of LDS); engine=ENGINE_DFA_GLOBAL leaves every table in HBM/L2.  RRegexError names the index of a member that does not
    parse or whose forward search automaton does not determinise."""

    def __init__(self, patterns, engine=None, max_rows=0, device=0):
        pats = [p.encode("latin-1") if isinstance(p, str) else bytes(p) for p in patterns]
        self.patterns, self.device = pats, device
        self._h = C.c_void_p()
        arr = (C.c_char_p * max(len(pats), 1))(*pats)
        _check(_L.rrx_multi_compile_ex(C.cast(arr, C.c_void_p), len(pats), ENGINE_AUTO if engine is None else engine, max_rows, C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None) and _L is not None:
            _L.rrx_multi_free(self._h)
            self._h = None

    def __len__(self):
        return _L.rrx_multi_patterns(self._h)

    @property
    def groups(self):
        """The number of groups, i.e. of launches per call."""
        return _L.rrx_multi_groups(self._h)

    def group_mask(self, g):
        """The members of group g as a bit mask; the groups' masks partition the set."""
        return _L.rrx_multi_group_mask(self._h, g)

    def group_states(self, g):
        """The rows of group g's product table."""
        return _L.rrx_multi_group_states(self._h, g)

    def program(self, g):
        """Group g's table as words (numpy uint32): [nstates, ncls, start, first_hit, full], cls[256], next[nstates][ncls],
        mask[nstates]; None for a group that is not there."""
        import numpy as np
        n = _L.rrx_multi_program_words(self._h, g, None, 0)
        if not n:
            return None
        out = np.zeros(n, dtype=np.uint32)
        _L.rrx_multi_program_words(self._h, g, C.c_void_p(out.ctypes.data), n)
        return out

    @staticmethod
    def _masks(n, device, out):
        import torch
        return _out(out, n, torch.int32, device)

    def contains_extents(self, data, offsets, trim=0, out=None, stream=None):
        """Item i = data[offsets[i] : offsets[i+1] - trim] -> an int32 tensor of n masks, bit k = the item contains a match of
        patterns[k] (rrx_multi_contains_extents).  Every word is written.  Asynchronous on `stream`."""
        n, d, b, o = _batch(data, offsets)
        with _on(d, stream):
            out = self._masks(n, data.device, out)
            _check(_L.rrx_multi_contains_extents(self._h, d, b, o, n, trim, _ptr(out), _stream_ptr(stream)))
        return out

    def contains_items(self, items, out=None, stream=None):
        """The same for an indexed batch (rrx_multi_contains_items)."""
        with _on(items.device, stream):
            out = self._masks(items.num_items, items.data.device, out)
            _check(_L.rrx_multi_contains_items(self._h, items._h, _ptr(out), _stream_ptr(stream)))
        return out

    def contains_corpus(self, corpus, out=None, stream=None):
        """Line i of the corpus, without its '\\n', as the item -> an int32 tensor of corpus.num_lines masks, bit k = the line contains
        a match of patterns[k] (rrx_multi_contains_corpus: a lane per stripe of the text).  Every word is written.  counts() and
        plane() apply; a plane has the layout of RRegex.contains_corpus_bits.  Asynchronous on `stream`."""
        with _on(corpus.device, stream):
            out = self._masks(corpus.num_lines, corpus.data.device, out)
            if out.numel():                        # (a corpus without lines: no word to write, and the entry refuses a null d_mask)
                _check(_L.rrx_multi_contains_corpus(self._h, corpus._h, _ptr(out), _stream_ptr(stream)))
        return out

    def counts(self, masks, stream=None):
        """Per pattern, the number of masks that have its bit (rrx_multi_counts) -> an int64 device tensor of len(self) totals.
        Asynchronous on `stream`."""
        import torch
        assert masks.is_cuda and masks.dtype == torch.int32 and masks.is_contiguous()
        with _on(masks.device.index, stream):
            counts = torch.empty(32, dtype=torch.int64, device=masks.device)
            _check(_L.rrx_multi_counts(masks.device.index, _ptr(masks), masks.numel(), _ptr(counts), _stream_ptr(stream)))
        return counts[:len(self)]

    def plane(self, masks, k, out=None, stream=None):
        """Bit k of every mask as a bitmap in the layout of RRegex.contains_extents_bits (rrx_multi_plane): ceil(n / 32) int32
        words, so that bitmap_count applies.  Asynchronous on `stream`."""
        import torch
        assert masks.is_cuda and masks.dtype == torch.int32 and masks.is_contiguous()
        n = masks.numel()
        nw = (n + 31) // 32
        with _on(masks.device.index, stream):
            out = _out(out, nw, torch.int32, masks.device)
            _check(_L.rrx_multi_plane(masks.device.index, _ptr(masks), n, k, _ptr(out), _stream_ptr(stream)))
        return out
