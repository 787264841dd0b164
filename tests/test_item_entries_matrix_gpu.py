"""The one-call entries that count, scan, read a total back and fill - rrx_search_all_extents / _items, rrx_search_all_longest_*,
rrx_replace_all_longest_*, rrx_extract_all_longest_*, rrx_split_longest_* and rrx_search_all on a corpus with a pattern that accepts
the empty string - as one matrix: family x form (_extents, _items) x batch (0, 1 and 5 items of at most 16 bytes, trim 0 and 1) x
pattern (an ordinary one, one that accepts the empty string, the empty language) x cap (0, total - 1, total; the pieces also at
pieces_cap = npieces - 1).  What these entries share is host code - the tables step, the empty batch, the scan with entry 0 zeroed,
the total and the flag word read back, the cap rule -, and nothing in it depends on the size of the batch: the large batches, the
alignments and the kernels' own edges are the business of the test files of each family.

Expected values: the oracle's iterated brute force (test_search_all_items_lowering / test_search_all_longest_items_lowering:
want_for), the splice rule and the pieces rule on those lists.  Every output array is poisoned between guard words, whatever lies at
or beyond a cap must still hold the poison, and the _items form must leave every buffer byte for byte as the _extents form does."""
import ctypes as C

import numpy as np
import pytest

import roaringregex_amd as rr
from test_pieces_items_lowering import pieces_rule
from test_replace_items_lowering import splice
from test_search_all_items_lowering import want_for as lazy_want_for
from test_search_all_longest_items_lowering import pack, want_for as longest_want_for

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_pieces_items_gpu import Words  # noqa: E402  (these need torch)
from test_replace_items_gpu import Guarded, ptr  # noqa: E402
from test_search_corpus_gpu import Want, device_corpus, search_all_once  # noqa: E402

BATCHES = {0: [], 1: [b"abcabbc;ab"], 5: [b"", b"abc", b"zabbcab", b"aab abbbc;abc", b"bbb"]}
PATTERNS = ("ab+c", "a*", "[]")                     # an ordinary pattern, one that accepts the empty string, the empty language
REP = b"<>"
ROOM = 8                                            # slots behind the last match, poisoned like the rest


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    assert all(len(it) <= 16 for items in BATCHES.values() for it in items)


def caps_of(total):
    return sorted({0, max(total - 1, 0), total})


def batch_on_device(items, trim):
    text, offs = pack(items, trim, lead=trim * 3, seed=len(items))
    dev = torch.from_numpy(text).cuda() if len(text) else torch.empty(0, dtype=torch.uint8, device="cuda")
    doff = torch.from_numpy(offs).cuda()
    return dev, doff, rr.Items(dev, doff, trim=trim)


def both_forms(call, what):
    """call(indexed) -> the buffers it checked; the indexed batch must leave each of them as the offsets array does."""
    plain, indexed = call(False), call(True)
    for a, b in zip(plain, indexed):
        assert torch.equal(a.buf, b.buf), (what, "the _items form and the _extents form differ")


def search_all_cell(entry, r, dev, doff, handle, trim, want_lists, cap, indexed, what):
    L, s = rr._L, rr._stream_ptr(None)
    n = doff.numel() - 1
    first = np.concatenate([[0], np.cumsum([len(w) for w in want_lists], dtype=np.int64)]).astype(np.int64)
    pairs = np.array([x for w in want_lists for x in w], dtype=np.int32).reshape(-1, 2)
    total = len(pairs)
    d_first, d_start, d_end, tot = Words(n + 1, torch.int64), Words(total + ROOM, torch.int32), Words(total + ROOM, torch.int32), C.c_size_t(99)
    if indexed:
        rr._check(getattr(L, "rrx_%s_items" % entry)(r._h, handle._h, d_first.ptr, d_start.ptr, d_end.ptr, cap, C.byref(tot), s))
    else:
        rr._check(getattr(L, "rrx_%s_extents" % entry)(r._h, 0, ptr(dev), ptr(doff), n, trim, d_first.ptr, d_start.ptr, d_end.ptr, cap, C.byref(tot), s))
    torch.cuda.synchronize()
    what = what + ("indexed", indexed)
    print(what, "total", tot.value, "want", total)
    assert tot.value == total, (what, "*total", tot.value, total)
    assert np.array_equal(d_first.written(what), first), (what, "d_first is complete at every cap")
    k = min(cap, total)
    assert np.array_equal(d_start.written(what + ("a slot at or beyond the cap was written",), k), pairs[:k, 0]), (what, "d_start")
    assert np.array_equal(d_end.written(what + ("a slot at or beyond the cap was written",), k), pairs[:k, 1]), (what, "d_end")
    return d_first, d_start, d_end


@pytest.mark.parametrize("trim", [0, 1])
@pytest.mark.parametrize("nitems", sorted(BATCHES))
@pytest.mark.parametrize("entry", ["search_all", "search_all_longest"])
def test_search_all_one_call(entry, nitems, trim):
    items = BATCHES[nitems]
    dev, doff, handle = batch_on_device(items, trim)
    for p in PATTERNS:
        r = rr.RRegex(p)
        want_lists = (lazy_want_for if entry == "search_all" else longest_want_for)(p, items)
        for cap in caps_of(sum(len(w) for w in want_lists)):
            what = (entry, p, "items", nitems, "trim", trim, "cap", cap)
            both_forms(lambda indexed: search_all_cell(entry, r, dev, doff, handle, trim, want_lists, cap, indexed, what), what)


def replace_cell(r, dev, doff, handle, trim, want, cap, indexed, what):
    L, s = rr._L, rr._stream_ptr(None)
    n, total = doff.numel() - 1, len(want[0])
    out_off, g, tot = Words(n + 1, torch.int64), Guarded(total + ROOM), C.c_size_t(99)
    d_out = ptr(g.d_out) if cap else None
    if indexed:
        rr._check(L.rrx_replace_all_longest_items(r._h, handle._h, REP, len(REP), out_off.ptr, d_out, cap, C.byref(tot), s))
    else:
        rr._check(L.rrx_replace_all_longest_extents(r._h, 0, ptr(dev), ptr(doff), n, trim, REP, len(REP), out_off.ptr, d_out, cap, C.byref(tot), s))
    torch.cuda.synchronize()
    what = what + ("indexed", indexed)
    print(what, "total", tot.value, "want", total)
    assert tot.value == total, (what, "*total", tot.value, total)
    assert np.array_equal(out_off.written(what), want[1]), (what, "d_out_off is complete at every cap")
    if total and total <= cap:
        got = g.written(what)
        assert np.array_equal(got[:total], want[0]) and (got[total:] == 0x5A).all(), (what, "the column, and nothing behind it")
    else:
        g.untouched(what + ("a column beyond the cap: not a byte of it is written",))
    return out_off, g


@pytest.mark.parametrize("trim", [0, 1])
@pytest.mark.parametrize("nitems", sorted(BATCHES))
def test_replace_all_longest(nitems, trim):
    items = BATCHES[nitems]
    dev, doff, handle = batch_on_device(items, trim)
    for p in PATTERNS:
        r = rr.RRegex(p)
        outs = [splice(it, w, REP) for it, w in zip(items, longest_want_for(p, items))]
        want = (np.frombuffer(b"".join(outs), dtype=np.uint8), np.concatenate([[0], np.cumsum([len(o) for o in outs], dtype=np.int64)]).astype(np.int64))
        for cap in caps_of(len(want[0])):
            what = ("replace_all_longest", p, "items", nitems, "trim", trim, "cap", cap)
            both_forms(lambda indexed: replace_cell(r, dev, doff, handle, trim, want, cap, indexed, what), what)


def pieces_cell(gaps, r, dev, doff, handle, trim, want, pieces_cap, cap, indexed, what):
    L, s = rr._L, rr._stream_ptr(None)
    want_bytes, want_piece_off, want_list_off = want
    n, npieces, total = doff.numel() - 1, len(want_piece_off) - 1, len(want_bytes)
    list_off, piece_off, g = Words(n + 1, torch.int64), Words(npieces + 1 + ROOM, torch.int64), Guarded(total + ROOM)
    npc, tot = C.c_size_t(99), C.c_size_t(99)
    d_out = ptr(g.d_out) if cap else None
    name = "rrx_split_longest_" if gaps else "rrx_extract_all_longest_"
    if indexed:
        rr._check(getattr(L, name + "items")(r._h, handle._h, list_off.ptr, piece_off.ptr, pieces_cap, d_out, cap, C.byref(npc), C.byref(tot), s))
    else:
        rr._check(getattr(L, name + "extents")(r._h, 0, ptr(dev), ptr(doff), n, trim, list_off.ptr, piece_off.ptr, pieces_cap, d_out, cap, C.byref(npc),
                                               C.byref(tot), s))
    torch.cuda.synchronize()
    what = what + ("indexed", indexed)
    print(what, "npieces", npc.value, "want", npieces, "total", tot.value, "want", total)
    assert (npc.value, tot.value) == (npieces, total), (what, npc.value, tot.value, npieces, total)
    assert np.array_equal(list_off.written(what), want_list_off), (what, "d_list_off is complete at every cap")
    if npieces <= pieces_cap:
        assert np.array_equal(piece_off.written(what, npieces + 1), want_piece_off), (what, "d_piece_off")
    else:
        piece_off.written(what + ("more pieces than pieces_cap: d_piece_off is not written",), 0)
    if npieces <= pieces_cap and total and total <= cap:
        got = g.written(what)
        assert np.array_equal(got[:total], want_bytes) and (got[total:] == 0x5A).all(), (what, "the column, and nothing behind it")
    else:
        g.untouched(what + ("a column beyond either cap: not a byte of it is written",))
    return list_off, piece_off, g


@pytest.mark.parametrize("trim", [0, 1])
@pytest.mark.parametrize("nitems", sorted(BATCHES))
@pytest.mark.parametrize("gaps", [False, True], ids=["extract_all_longest", "split_longest"])
def test_pieces_all_longest(gaps, nitems, trim):
    items = BATCHES[nitems]
    dev, doff, handle = batch_on_device(items, trim)
    for p in PATTERNS:
        r = rr.RRegex(p)
        per = [pieces_rule(it, w, gaps) for it, w in zip(items, longest_want_for(p, items))]
        lens = [len(x) for pieces in per for x in pieces]
        want = (np.frombuffer(b"".join(b"".join(pieces) for pieces in per), dtype=np.uint8),
                np.concatenate([[0], np.cumsum(lens, dtype=np.int64)]).astype(np.int64),
                np.concatenate([[0], np.cumsum([len(pieces) for pieces in per], dtype=np.int64)]).astype(np.int64))
        npieces, total = len(lens), len(want[0])
        for pieces_cap in sorted({max(npieces - 1, 0), npieces}):
            for cap in caps_of(total):
                what = ("split_longest" if gaps else "extract_all_longest", p, "items", nitems, "trim", trim, "pieces_cap", pieces_cap, "cap", cap)
                both_forms(lambda indexed: pieces_cell(gaps, r, dev, doff, handle, trim, want, pieces_cap, cap, indexed, what), what)


@pytest.mark.parametrize("nlines", sorted(BATCHES))
@pytest.mark.parametrize("pattern", ["a*", "x?y?z?"])
def test_search_all_on_a_corpus_with_a_pattern_that_accepts_the_empty_string(pattern, nlines):
    """The lines of the corpus are the items of the batches (a corpus has one form and its separator is the '\\n')."""
    lines = BATCHES[nlines]
    assert not any(b"\n" in ln for ln in lines)
    corpus = device_corpus(np.frombuffer(b"".join(ln + b"\n" for ln in lines), dtype=np.uint8))
    assert corpus.num_lines == nlines
    all_want = lazy_want_for(pattern, lines)
    assert all_want == [[(k, k) for k in range(len(ln) + 1)] for ln in lines]
    want = Want([w[0] for w in all_want], all_want)
    r = rr.RRegex(pattern)
    for cap in caps_of(want.total):
        print(("search_all, corpus", pattern, "lines", nlines, "cap", cap, "total", want.total))
        search_all_once(r, corpus, want, cap, ("search_all, corpus", pattern, "lines", nlines))
