"""rrx_pieces_sizes / _fill, rrx_extract_all_longest_* and rrx_split_longest_* on the device: the list<binary> column of every item's
matches (extract_all) or of what lies between them (split) - list offsets, piece offsets and bytes - against the rule on the oracle's
lists (short items: the CPU test's patterns, items and expected lists), against the rule on the lists the device itself found taken
earliest-end-first, against re.findall / re.split where Python's greedy search names the leftmost-longest list, and against the
clamped rule on lists that are not the items'.  Every output array stands between 64 poisoned bytes or words in front and 64 behind,
which must come back unchanged.  Expected columns are built on the host."""
import ctypes as C
import random
import re

import numpy as np
import pytest

import roaringregex_amd as rr
from test_pieces_items_lowering import pieces_rule
from test_replace_items_lowering import csr_lists
from test_search_all_longest_items_lowering import GREEDY_ALL_RE, finditer_all, pack, reference_all
from test_search_all_longest_items_gpu import POOL, pooled_batch, to_dev
from test_replace_items_gpu import Guarded, at_residue, host_lists, pooled_column, ptr

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD = 64
POISON_WORD = {torch.int32: 0x5A5A5A5A, torch.int64: 0x5A5A5A5A5A5A5A5A}
MAX_LANES_SIZES = 512 * 1024                        # device.hpp: kReplaceMaxBlocks workgroups of 1024 lanes, then the sizes grid strides
PIECES_CHUNK = 4096                                 # device.hpp: kPiecesChunk, the bytes of output a wave takes at a time
PIECES_GRID_WAVES = 512 * 16                        # device.hpp: kPiecesMaxBlocks workgroups of 1024 lanes = 16 waves each, always
MATCHES, GAPS = False, True


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"


class Words:
    """n words of an output array between GUARD poisoned words in front and GUARD behind, all of it poisoned."""

    def __init__(self, n, dtype):
        self.n, self.poison = n, POISON_WORD[dtype]
        self.buf = torch.full((GUARD + n + GUARD,), self.poison, dtype=dtype, device="cuda")
        self.view = self.buf[GUARD:GUARD + n]
        self.ptr = C.c_void_p(self.buf.data_ptr() + GUARD * self.buf.element_size())        # (never null, also for n == 0)

    def written(self, what, count=None):
        """The first `count` words (all n by default), after the check that nothing else changed."""
        count = self.n if count is None else count
        host = self.buf.cpu().numpy()
        assert (host[:GUARD] == self.poison).all() and (host[GUARD + count:] == self.poison).all(), (what, "a word outside the array was written")
        return host[GUARD:GUARD + count]


def expected_column(items, lists, gaps, out_first=0):
    """(bytes, piece_off from out_first, list_off) of the pieces the rule names."""
    per = [pieces_rule(it, w, gaps) for it, w in zip(items, lists)]
    lens = np.array([len(x) for p in per for x in p], dtype=np.int64)
    piece_off = (out_first + np.concatenate([[0], np.cumsum(lens)])).astype(np.int64)
    list_off = np.concatenate([[0], np.cumsum([len(p) for p in per])]).astype(np.int64)
    return np.frombuffer(b"".join(b"".join(p) for p in per), dtype=np.uint8), piece_off, list_off


def assert_column(got_bytes, got_piece_off, got_list_off, want, what):
    assert np.array_equal(got_list_off, want[2]), (what, "list_off", got_list_off[:8], want[2][:8])
    assert np.array_equal(got_piece_off, want[1]), (what, "piece_off", int(np.nonzero(got_piece_off != want[1])[0][0]) if len(got_piece_off) == len(want[1]) else "length")
    assert len(got_bytes) == len(want[0]), (what, len(got_bytes), len(want[0]))
    bad = np.nonzero(got_bytes != want[0])[0]
    assert bad.size == 0, (what, "first bad byte", int(bad[0]), "piece", int(np.searchsorted(want[1], bad[0] + want[1][0], side="right")) - 1,
                           bytes(got_bytes[bad[0]:bad[0] + 8]), bytes(want[0][bad[0]:bad[0] + 8]))


def lists_to_dev(lists, first0=0):
    """[[(s, e)]] per item -> device (first[n + 1], start, end); the slots in front of first0 hold values no item has."""
    first, start, end = csr_lists(lists, first0)
    start = [0x7FFFFFF0 if s is None else s for s in start]
    end = [0x7FFFFFF1 if e is None else e for e in end]
    as32 = lambda v: torch.from_numpy(np.array(v, dtype=np.uint32).view(np.int32).copy()).cuda() if v else torch.empty(0, dtype=torch.int32, device="cuda")
    return torch.from_numpy(np.array(first, dtype=np.int64)).cuda(), as32(start), as32(end)


def generic_pair(dev, doff, trim, first, start, end, gaps, want, what, out_first=0, out_mis=0):
    """sizes, the prefix with torch, fill - through the C entries, every array of the caller's poisoned; want = expected_column(...)."""
    L, s = rr._L, rr._stream_ptr(None)
    n, npieces, total = doff.numel() - 1, len(want[1]) - 1, len(want[0])
    if not start.numel():
        start = end = torch.zeros(1, dtype=torch.int32, device="cuda")
    list_off, length, src = Words(n + 1, torch.int64), Words(npieces, torch.int32), Words(npieces, torch.int64)
    rr._check(L.rrx_pieces_sizes(0, ptr(doff), n, trim, ptr(first), ptr(start), ptr(end), 1 if gaps else 0, list_off.ptr, length.ptr, src.ptr, s))
    got_list_off = list_off.written(what + ("list_off",))
    lens = length.written(what + ("piece_len",)).astype(np.int64) & 0xFFFFFFFF
    src.written(what + ("piece_src",))
    piece_off = torch.full((npieces + 1,), out_first, dtype=torch.int64, device="cuda")
    if npieces:
        piece_off[1:] += torch.cumsum(length.view.to(torch.int64) & 0xFFFFFFFF, dim=0)
    assert int(lens.sum()) == total, (what, "total", int(lens.sum()), total)
    g = Guarded(total, lead=out_first, mis=out_mis)
    rr._check(L.rrx_pieces_fill(0, ptr(dev), src.ptr, ptr(piece_off), npieces, ptr(g.d_out) if total else None, s))
    torch.cuda.synchronize()
    got = g.written(what)
    assert_column(got, piece_off.cpu().numpy(), got_list_off, want, what)
    return got


def one_call(r, dev, doff, trim, gaps, want, what, handle=None, out_mis=0, pieces_cap=None, cap=None):
    """A one-call form on the offsets or on an indexed batch, by default with the exact caps: the cap protocol in full."""
    L, s = rr._L, rr._stream_ptr(None)
    n, npieces, total = doff.numel() - 1, len(want[1]) - 1, len(want[0])
    pieces_cap = npieces if pieces_cap is None else pieces_cap
    cap = total if cap is None else cap
    list_off, piece_off, g = Words(n + 1, torch.int64), Words(pieces_cap + 1, torch.int64), Guarded(total, mis=out_mis)
    npc, tot = C.c_size_t(99), C.c_size_t(99)
    d_out = ptr(g.d_out) if cap else None
    if handle is None:
        fn = L.rrx_split_longest_extents if gaps else L.rrx_extract_all_longest_extents
        rr._check(fn(r._h, 0, ptr(dev), ptr(doff), n, trim, list_off.ptr, piece_off.ptr, pieces_cap, d_out, cap, C.byref(npc), C.byref(tot), s))
    else:
        fn = L.rrx_split_longest_items if gaps else L.rrx_extract_all_longest_items
        rr._check(fn(r._h, handle._h, list_off.ptr, piece_off.ptr, pieces_cap, d_out, cap, C.byref(npc), C.byref(tot), s))
    torch.cuda.synchronize()
    what = what + ("pieces_cap", pieces_cap, "cap", cap)
    assert (npc.value, tot.value) == (npieces, total), (what, npc.value, tot.value, npieces, total)
    assert np.array_equal(list_off.written(what), want[2]), (what, "d_list_off is complete either way")
    if npieces <= pieces_cap:
        assert np.array_equal(piece_off.written(what, npieces + 1), want[1]), (what, "piece_off")
    else:
        piece_off.written(what, 0)
    if npieces <= pieces_cap and total <= cap:
        got = g.written(what)
        bad = np.nonzero(got != want[0])[0]
        assert bad.size == 0, (what, "first bad byte", int(bad[0]))
    else:
        g.untouched(what)


def all_forms(r, dev, doff, trim, items, lists, what, handle=None, out_mis=0):
    """Both modes through the generic pair on the device's own leftmost-longest lists and through the one-call forms."""
    found = r.search_all_longest_extents_fused(dev, doff, trim=trim)
    for gaps in (MATCHES, GAPS):
        want = expected_column(items, lists, gaps, out_first=7)
        generic_pair(dev, doff, trim, *found, gaps, want, what + ("generic", gaps), out_first=7, out_mis=out_mis)
        want = expected_column(items, lists, gaps)
        one_call(r, dev, doff, trim, gaps, want, what + ("one call", gaps), out_mis=(out_mis + 1) % 4)
        if handle is not None:
            one_call(r, dev, doff, trim, gaps, want, what + ("one call, indexed", gaps), handle=handle, out_mis=(out_mis + 2) % 4)


def test_short_items_against_the_brute_force():
    for p, items, want_lists in reference_all():
        r = rr.RRegex(p)
        for trim in (0, 1):
            dev, doff = to_dev(*pack(items, trim, lead=3 + trim, seed=len(items) + trim))
            assert int(doff[0]) != 0
            handle = rr.Items(dev, doff, trim=trim)
            longest = r.search_all_longest_extents_fused(dev, doff, trim=trim)
            assert host_lists(*longest) == [list(w) for w in want_lists], (p[:30], "the device's lists are the oracle's")
            lazy = r.search_all_extents_fused(dev, doff, trim=trim)
            lazy_lists = host_lists(*lazy)
            what = (p[:30], "trim", trim)
            for gaps in (MATCHES, GAPS):
                want = expected_column(items, want_lists, gaps, out_first=5)
                got = generic_pair(dev, doff, trim, *longest, gaps, want, what + ("longest lists", gaps), out_first=5, out_mis=1 + trim)
                if gaps:                                           # the same bytes as replace's fill with an empty replacement, byte for byte
                    out, _ = rr.replace_matches(dev, doff, *longest, b"", trim=trim)
                    assert np.array_equal(out.cpu().numpy(), got), (what, "rrx_replace_matches_fill at rep_len 0")
                generic_pair(dev, doff, trim, *lazy, gaps, expected_column(items, lazy_lists, gaps), what + ("earliest-end-first lists", gaps), out_mis=3)
                want = expected_column(items, want_lists, gaps)
                one_call(r, dev, doff, trim, gaps, want, what + ("one call", gaps))
                one_call(r, dev, doff, trim, gaps, want, what + ("one call, indexed", gaps), handle=handle, out_mis=2)
                # the Python layer: the same columns, also where the first caps were too small
                columns = ((rr.pieces_of_matches(dev, doff, *longest, gaps=gaps, trim=trim),)
                           + ((r.split_longest_extents(dev, doff, trim=trim), r.split_longest_extents(dev, doff, trim=trim, cap=1, pieces_cap=1),
                               r.split_longest_items(handle)) if gaps else
                              (r.extract_all_longest_extents(dev, doff, trim=trim), r.extract_all_longest_extents(dev, doff, trim=trim, cap=1, pieces_cap=1),
                               r.extract_all_longest_items(handle))))
                for out, piece_off, list_off in columns:
                    assert_column(out.cpu().numpy(), piece_off.cpu().numpy(), list_off.cpu().numpy(), want, what + ("python", gaps))
    for p, item, matches, gaps in (("[0-9]+", b"a1 22 333", [b"1", b"22", b"333"], [b"a", b" ", b" ", b""]),
                                   ("a*", b"baab", [b"", b"aa", b"", b""], [b"", b"b", b"", b"b", b""])):
        dev, doff = to_dev(*pack([item] * 3, 1, lead=3))
        for got, want in ((rr.RRegex(p).extract_all_longest_extents(dev, doff, trim=1), matches), (rr.RRegex(p).split_longest_extents(dev, doff, trim=1), gaps)):
            out, piece_off, list_off = (t.cpu().numpy() for t in got)
            assert [out[piece_off[k]:piece_off[k + 1]].tobytes() for k in range(len(piece_off) - 1)] == want * 3, (p, "named case")
            assert list_off.tolist() == [0, len(want), 2 * len(want), 3 * len(want)]


def pooled_expected(per, idx, out_first=0):
    """The column of a batch drawn from a pool by `idx`, from the pieces per pool item (numpy: the batch may pass half a million)."""
    data, _ = pooled_column([b"".join(p) for p in per], idx)
    cnt = np.array([len(p) for p in per], dtype=np.int64)
    flat = np.array([len(x) for p in per for x in p], dtype=np.int64)
    poff = np.concatenate([[0], np.cumsum(cnt)])[:-1]
    c = cnt[idx]
    list_off = np.concatenate([[0], np.cumsum(c)]).astype(np.int64)
    src = np.arange(int(list_off[-1]), dtype=np.int64) - np.repeat(list_off[:-1], c) + np.repeat(poff[idx], c)
    piece_off = (out_first + np.concatenate([[0], np.cumsum(flat[src])])).astype(np.int64)
    return data, piece_off, list_off


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, MAX_LANES_SIZES + 65])
def test_batch_sizes(n):
    """The sizes kernel's edges: wave edges, workgroup edges and more items than one pass of its grid holds; trim 3 is larger than
    some items (region = item + ';')."""
    p, trim, lead = "ab+c", 3, 16
    r = rr.RRegex(p)
    trimmed = [(it + b";")[:max(len(it) + 1 - trim, 0)] for it in POOL]
    assert len(POOL) == 14 and sum(not t for t in trimmed) >= 3
    text, off, idx = pooled_batch(n, 40 + n % 7, lead)
    dev, doff = to_dev(text, off)
    found = r.search_all_longest_extents_fused(dev, doff, trim=trim)
    handle = rr.Items(dev, doff, trim=trim) if n <= 1025 else None
    for gaps in (MATCHES, GAPS):
        per = [pieces_rule(it, finditer_all(p, it), gaps) for it in trimmed]
        assert per == [re.split(GREEDY_ALL_RE[p], it) if gaps else re.findall(GREEDY_ALL_RE[p], it) for it in trimmed]
        generic_pair(dev, doff, trim, *found, gaps, pooled_expected(per, idx, out_first=9), ("batch", n, gaps), out_first=9, out_mis=n % 4)
        want = pooled_expected(per, idx)
        one_call(r, dev, doff, trim, gaps, want, ("batch", n, gaps, "one call"), out_mis=(n + 1) % 4)
        if handle is not None:
            one_call(r, dev, doff, trim, gaps, want, ("batch", n, gaps, "one call, indexed"), handle=handle)


def chopped(text, rng, longest=37):
    """`text` cut into items of 0 .. `longest` bytes."""
    items, at = [], 0
    while at < len(text):
        k = rng.randrange(longest + 1)
        items.append(text[at:at + k])
        at += k
    return items or [b""]


def test_fill_edges_small_totals_and_residues():
    """Output totals of 1 .. 5 bytes, around one chunk and beyond two, d_out + d_piece_off[0] at all four residues and d_bytes at
    1, 2, 3 mod 4: the source and destination residues differ in every combination; items without matches through GAPS (a piece per
    item, some empty), then with matches through both modes."""
    rng = random.Random(61)
    alphabet = b"abcxyz 0189"
    for total in (1, 2, 3, 4, 5, PIECES_CHUNK - 1, PIECES_CHUNK, PIECES_CHUNK + 1, 2 * PIECES_CHUNK + 3):
        text = bytes(rng.choice(alphabet) for _ in range(total))
        items = chopped(text, rng)
        host_text, offs = pack(items, 1, lead=0)
        for bytes_mis in (1, 2, 3):
            dev, doff = at_residue(host_text, bytes_mis), torch.from_numpy(offs).cuda()
            assert dev.data_ptr() % 4 == bytes_mis
            for out_mis in range(4):
                lists = [[] for _ in items]
                want = expected_column(items, lists, GAPS, out_first=out_mis + 4 * bytes_mis)
                assert len(want[0]) == total
                # (d_out at 1, 2, 3 mod 4; out_first moves d_out + lo through all four residues for each of them)
                generic_pair(dev, doff, 1, *lists_to_dev(lists), GAPS, want, ("total", total, bytes_mis, out_mis), out_first=out_mis + 4 * bytes_mis,
                             out_mis=bytes_mis)
        # the same text as ONE item with matches: the pieces of both modes cut it at other places
        lists = [[(m.start(), m.end()) for m in re.finditer(rb"[0-9]+|c", text)]]
        host_text, offs = pack([text], 0, lead=2)
        dev, doff = at_residue(host_text, total % 3 + 1), torch.from_numpy(offs).cuda()
        for gaps in (MATCHES, GAPS):
            for out_mis in range(4):
                generic_pair(dev, doff, 0, *lists_to_dev(lists, first0=2), gaps, expected_column([text], lists, gaps, out_first=1), ("one item", total, gaps, out_mis),
                             out_first=1, out_mis=out_mis)


def test_fill_edges_chunk_boundaries_and_empty_pieces():
    # a piece boundary exactly on a chunk boundary, at every residue of d_out + lo: the chunks are cut at aligned ADDRESSES
    for mis in range(4):
        items = [b"k" * (PIECES_CHUNK - mis), b"lmnopqrstu", b"v" * PIECES_CHUNK, b"w"]
        lists = [[] for _ in items]
        dev, doff = to_dev(*pack(items, 1, lead=1))
        generic_pair(dev, doff, 1, *lists_to_dev(lists), GAPS, expected_column(items, lists, GAPS, out_first=4), ("boundary", mis), out_first=4, out_mis=mis)
    # 1-byte pieces: [0-9] on digit strings - every byte of a dword is another piece
    rng = random.Random(62)
    items = [bytes(rng.choice(b"0123456789") for _ in range(k)) for k in (3000, 1, 0, 2 * PIECES_CHUNK + 1, 7)]
    lists = [[(k, k + 1) for k in range(len(it))] for it in items]
    assert lists == [[(m.start(), m.end()) for m in re.finditer(rb"[0-9]", it)] for it in items]
    dev, doff = to_dev(*pack(items, 1, lead=3))
    r = rr.RRegex("[0-9]")
    assert host_lists(*r.search_all_longest_extents_fused(dev, doff, trim=1)) == lists
    all_forms(r, dev, doff, 1, items, lists, ("1-byte pieces",), out_mis=1)
    # runs of 65 and of 5000 empty pieces whose offset is a chunk's first byte: a* on b's through MATCHES
    r = rr.RRegex("a*")
    for run in (65, 5000):
        items = [b"a" * (PIECES_CHUNK - 1), b"b" * (run - 2), b"aaaaaaa"]
        lists = [[(m.start(), m.end()) for m in re.finditer(rb"a*", it)] for it in items]
        want = expected_column(items, lists, MATCHES, out_first=1)
        assert int((want[1] == PIECES_CHUNK).sum()) == run + 1 and len(want[0]) == PIECES_CHUNK + 6
        dev, doff = to_dev(*pack(items, 0, lead=0))
        generic_pair(dev, doff, 0, *lists_to_dev(lists), MATCHES, want, ("empty pieces", run), out_first=1, out_mis=0)
        all_forms(r, dev, doff, 0, items, lists, ("empty pieces, all forms", run))
    # the run of 5000 empty pieces strictly INSIDE a chunk: more pieces begin in the chunk than the kPiecesChunk + 1 offsets behind its
    # first piece hold, so the kernel searches the whole rest of the offsets for the chunk's last piece (the CPU replay asserts the path)
    items = [b"a" * 100, b"b" * 4998, b"aaaaaaa"]
    lists = [[(m.start(), m.end()) for m in re.finditer(rb"a*", it)] for it in items]
    dev, doff = to_dev(*pack(items, 0, lead=0))
    for out_mis in (0, 3):
        want = expected_column(items, lists, MATCHES, out_first=2)
        assert len(want[0]) + 3 < PIECES_CHUNK and want[1][0 + PIECES_CHUNK + 1] <= want[1][-1] - 1, "piece_off[pa + chunk + 1] <= the chunk's last byte"
        generic_pair(dev, doff, 0, *lists_to_dev(lists), MATCHES, want, ("empty pieces inside a chunk", out_mis), out_first=2, out_mis=out_mis)
    # a batch whose MATCHES output is empty while it has pieces
    items = [b"bbb", b"", b"b" * 100] * 30
    lists = [[(k, k) for k in range(len(it) + 1)] for it in items]
    dev, doff = to_dev(*pack(items, 1, lead=1))
    want = expected_column(items, lists, MATCHES)
    assert len(want[0]) == 0 and len(want[1]) - 1 == sum(len(it) + 1 for it in items)
    all_forms(r, dev, doff, 1, items, lists, ("no bytes, many pieces",), handle=rr.Items(dev, doff, trim=1))


def test_one_piece_across_every_wave():
    """One item just over (waves of the grid) x chunk bytes through GAPS with two matches: three pieces, the middle one taken by every
    wave of the grid, the first waves a second chunk grid-stride - the case the division by output bytes exists for."""
    size = PIECES_GRID_WAVES * PIECES_CHUNK + 2 * PIECES_CHUNK + 5
    rng = np.random.default_rng(63)
    text = rng.integers(0, 256, size=size, dtype=np.uint8)
    lists = [[(1000, 1003), (size - 700, size - 3)]]
    item = text.tobytes()
    host_text, offs = pack([item], 1, lead=1)
    dev, doff = to_dev(host_text, offs)
    want = expected_column([item], lists, GAPS, out_first=2)
    assert want[2].tolist() == [0, 3] and np.diff(want[1]).tolist() == [1000, size - 700 - 1003, 3] and len(want[0]) > PIECES_GRID_WAVES * PIECES_CHUNK
    generic_pair(dev, doff, 1, *lists_to_dev(lists), GAPS, want, ("one long piece",), out_first=2, out_mis=3)
    want = expected_column([item], lists, MATCHES)
    generic_pair(dev, doff, 1, *lists_to_dev(lists), MATCHES, want, ("one long piece, matches",), out_mis=1)


def test_long_items():
    """One item of 60000 digits and blanks with more than 10000 matches, one match of 30 KB, a 100 KB item without a match, a batch
    of a single item; the expected columns from re.findall and re.split."""
    rng = random.Random(41)
    fill = b"xy zb" * 20001                                         # (no 'a', no digit: no pattern matches inside it)
    dense = bytes(rng.choice(b"0123456789   ") for _ in range(60000))
    assert len(finditer_all("[0-9]+", dense)) > 10000
    long_match = fill[:40000] + b"a" + b"b" * 30000 + b"c" + fill[:16] + b"abc"
    assert max(e - s for s, e in finditer_all("ab+c", long_match)) == 30002
    batches = (("[0-9]+", [dense, fill[:100000], b"12345" + fill[:65536] + b"678"]), ("[0-9]+", [dense]), ("[0-9]+", [fill[:100000]]),
               ("ab+c", [long_match, fill[:100000], b"abc" * 2000]), ("ab+c", [long_match]))
    for p, items in batches:
        r = rr.RRegex(p)
        lists = [finditer_all(p, it) for it in items]
        assert [pieces_rule(it, w, MATCHES) for it, w in zip(items, lists)] == [re.findall(GREEDY_ALL_RE[p], it) for it in items]
        assert [pieces_rule(it, w, GAPS) for it, w in zip(items, lists)] == [re.split(GREEDY_ALL_RE[p], it) for it in items]
        for trim, lead in ((0, 0), (1, 7)):
            dev, doff = to_dev(*pack(items, trim, lead, seed=trim))
            all_forms(r, dev, doff, trim, items, lists, (p, "long", len(items), trim), handle=rr.Items(dev, doff, trim=trim), out_mis=1 + trim)


def test_degenerate_cases():
    L, s = rr._L, rr._stream_ptr(None)
    r = rr.RRegex("ab+c")
    nothing = torch.empty(0, dtype=torch.uint8, device="cuda")
    zero = torch.zeros(1, dtype=torch.int64, device="cuda")
    empty = (np.empty(0, dtype=np.uint8), np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64))
    # nitems == 0 / npieces == 0: the generic entries write nothing, the one-call forms d_list_off[0] = d_piece_off[0] = 0
    g, w, v = Guarded(8), Words(4, torch.int32), Words(4, torch.int64)
    for mode in (0, 1):
        assert L.rrx_pieces_sizes(0, ptr(zero), 0, 0, ptr(zero), w.ptr, w.ptr, mode, v.ptr, w.ptr, v.ptr, s) == 0
    assert L.rrx_pieces_fill(0, None, v.ptr, v.ptr, 0, ptr(g.d_out), s) == 0
    torch.cuda.synchronize()
    g.untouched("empty batch")
    w.written("empty batch", 0)
    v.written("empty batch", 0)
    for rx in (r, rr.RRegex("a*"), rr.RRegex("[]")):
        for gaps in (MATCHES, GAPS):
            one_call(rx, nothing, zero, 0, gaps, empty, ("empty batch", rx.pattern, gaps), pieces_cap=3, cap=0)
            one_call(rx, nothing, zero, 0, gaps, empty, ("empty batch, indexed", rx.pattern, gaps), handle=rr.Items(nothing, zero))
        out, piece_off, list_off = rx.split_longest_extents(nothing, zero)
        assert out.numel() == 0 and piece_off.tolist() == [0] and list_off.tolist() == [0]
        out, piece_off, list_off = rr.pieces_of_matches(nothing, zero, zero, torch.empty(0, dtype=torch.int32, device="cuda"), torch.empty(0, dtype=torch.int32, device="cuda"))
        assert out.numel() == 0 and piece_off.tolist() == [0] and list_off.tolist() == [0]
    # a batch of empty items: split gives one empty piece each (a* too: its one empty match leaves two empty gaps), extract the matches
    off0 = torch.zeros(71, dtype=torch.int64, device="cuda")
    empties = [b""] * 70
    for rx, lists in ((r, [[]] * 70), (rr.RRegex("a*"), [[(0, 0)]] * 70), (rr.RRegex("[]"), [[]] * 70)):
        assert host_lists(*rx.search_all_longest_extents_fused(nothing, off0)) == [list(w) for w in lists]
        all_forms(rx, nothing, off0, 0, empties, lists, ("empty items", rx.pattern))
    # a pattern that accepts the empty string: re.findall / re.split; the empty language: no matches, every item one piece
    rng = random.Random(52)
    items = [bytes(rng.choice(b"aab") for _ in range(rng.randrange(0, 40))) for _ in range(150)] + [b"baab", b""]
    for trim, lead in ((0, 0), (1, 5), (2, 1)):
        dev, doff = to_dev(*pack(items, trim, lead))
        handle = rr.Items(dev, doff, trim=trim)
        lists = [[(m.start(), m.end()) for m in re.finditer(rb"a*", it)] for it in items]
        assert [pieces_rule(it, w, MATCHES) for it, w in zip(items, lists)] == [re.findall(rb"a*", it) for it in items]
        assert [pieces_rule(it, w, GAPS) for it, w in zip(items, lists)] == [re.split(rb"a*", it) for it in items]
        all_forms(rr.RRegex("a*"), dev, doff, trim, items, lists, ("a*", trim), handle=handle)
        all_forms(rr.RRegex("[]"), dev, doff, trim, items, [[]] * len(items), ("[]", trim), handle=handle)
    # a trim larger than every item: extract gives nothing, split one empty piece per item
    all_forms(r, dev, doff, 100, [b""] * len(items), [[]] * len(items), ("a trim larger than every item",))


def test_lists_that_are_not_the_items():
    """Starts and ends beyond the item, unordered, e < s: the column is the clamped rule's.  Neighbouring items hold other bytes, so
    a read outside the item would show in the output."""
    rng = random.Random(64)
    items = [bytes(rng.choice(b"abc" if k % 2 else b"xyz") for _ in range(rng.randrange(12))) for k in range(300)]
    lists = [[(rng.randrange(16), rng.randrange(16)) for _ in range(rng.randrange(4))] for _ in items]
    lists[5] = [(0xFFFFFFFF, 0xFFFFFFFF), (3, 1), (0, 0xFFFFFFFE)]
    assert any(e < s for w in lists for s, e in w) and any(s > len(it) for it, w in zip(items, lists) for s, e in w)
    for trim, lead in ((1, 3), (0, 0)):
        host_text, offs = pack(items, trim, lead)
        assert not (set(b"abcxyz") & set(host_text[:lead].tolist()))
        dev, doff = to_dev(host_text, offs)
        for gaps in (MATCHES, GAPS):
            want = expected_column(items, lists, gaps, out_first=2)
            assert len(want[0]) > 100
            generic_pair(dev, doff, trim, *lists_to_dev(lists, first0=3), gaps, want, ("hostile", trim, gaps), out_first=2, out_mis=3)


def test_the_cap_protocol():
    L, s = rr._L, rr._stream_ptr(None)
    p, items, want_lists = next(x for x in reference_all() if x[0] == "[ab]{1,2}b*a*")
    r = rr.RRegex(p)
    dev, doff = to_dev(*pack(items, 1, lead=1))
    handle = rr.Items(dev, doff, trim=1)
    n = len(items)
    for gaps in (MATCHES, GAPS):
        want = expected_column(items, want_lists, gaps)
        npieces, total = len(want[1]) - 1, len(want[0])
        assert npieces > 5 and total > 5
        for indexed in (None, handle):
            for pieces_cap in (npieces - 1, 0, npieces, npieces + 5):
                for cap in (total - 1, 0, total, total + 5):
                    one_call(r, dev, doff, 1, gaps, want, ("caps", gaps, indexed is not None), handle=indexed, pieces_cap=pieces_cap, cap=cap)
        w, npc, tot = Words(n + 1, torch.int64), C.c_size_t(0), C.c_size_t(0)
        fn = L.rrx_split_longest_extents if gaps else L.rrx_extract_all_longest_extents
        assert fn(r._h, 0, ptr(dev), ptr(doff), n, 1, w.ptr, w.ptr, 5, None, 5, C.byref(npc), C.byref(tot), s) == 2      # RRX_ERR_ARG: cap > 0 and no d_out
