"""rrx_bitmap_rank, rrx_filter_sizes, rrx_filter_corpus_sizes and rrx_filter_contains_* on the device, against the rule of
filter_cases.py alone: the rank of a bitmap, the (row, source, length) triples of the rows it selects - from an offsets array and, for
the lines of a corpus, from the text and the stripe index - the column rrx_pieces_fill writes from them, and the one-call forms with
their cap protocol.  Every output array stands between 64 poisoned words or bytes in front and 64 behind, which must come back
unchanged; the spare bits of every bitmap's last word hold garbage.  Expected columns are built on the host."""
import ctypes as C
import re

import numpy as np
import pytest

import filter_cases as F
import roaringregex_amd as rr

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD = 64
POISON = {torch.uint8: 0x5A, torch.int32: 0x5A5A5A5A, torch.int64: 0x5A5A5A5A5A5A5A5A}
ERR_UNSUPPORTED = 4


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"


class Guarded:
    """n elements of an output array between GUARD poisoned elements in front and GUARD behind, all of it poisoned."""

    def __init__(self, n, dtype):
        self.n, self.poison = n, POISON[dtype]
        self.buf = torch.full((GUARD + n + GUARD,), self.poison, dtype=dtype, device="cuda")
        self.view = self.buf[GUARD:GUARD + n]
        self.ptr = C.c_void_p(self.buf.data_ptr() + GUARD * self.buf.element_size())        # (never null, also for n == 0)

    def written(self, what, count=None):
        """The first `count` elements (all n by default), after the check that nothing else changed."""
        count = self.n if count is None else count
        host = self.buf.cpu().numpy()
        assert (host[:GUARD] == self.poison).all() and (host[GUARD + count:] == self.poison).all(), (what, "an element outside the array was written")
        return host[GUARD:GUARD + count]


def ptr(t):
    return C.c_void_p(t.data_ptr())


def dev_bytes(data):
    """The bytes on the device, 16-byte aligned, never an empty tensor."""
    a = np.frombuffer(bytes(data) + b"\x00", dtype=np.uint8)
    return torch.from_numpy(a.copy()).cuda()[:len(data)]


def dev_words(words):
    """A bitmap on the device (one word more than it has: never an empty tensor)."""
    a = np.concatenate([np.asarray(words, dtype=np.uint32), np.array([0xDEADBEEF], dtype=np.uint32)])
    return torch.from_numpy(a.view(np.int32).copy()).cuda()


def stream():
    return rr._stream_ptr(None)


# ---------------------------------------------------------------------------------------------------------------- rank
def check_rank(words, nbits, what):
    L = rr._L
    nw = (nbits + 31) // 32
    bits = dev_words(words)
    rw = L.rrx_bitmap_rank_words(nbits)
    for invert in (0, 1):
        rank = Guarded(rw, torch.int64)
        rr._check(L.rrx_bitmap_rank(0, ptr(bits), nbits, invert, rank.ptr, rw, stream()))
        torch.cuda.synchronize()
        got = rank.written((what, invert)).view(np.uint64)[:nw + 1]
        want = F.rank_rule(words, nbits, bool(invert))
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (what, "invert", invert, "first bad entry", int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))


def rank_bitmaps(nbits, rng):
    nw = (nbits + 31) // 32
    yield "all zero", np.zeros(nw, dtype=np.uint32)
    yield "all one", np.full(nw, 0xFFFFFFFF, dtype=np.uint32)
    yield "random", rng.integers(0, 1 << 32, size=nw, dtype=np.uint64).astype(np.uint32)


@pytest.mark.parametrize("nbits", F.RANK_NBITS + tuple(32 * w for w in F.RANK_NWORDS) + tuple(32 * w - 13 for w in F.RANK_NWORDS))
def test_rank(nbits):
    """The bits of one word and of 64 words and their neighbours, and 4095, 4096 and 4097 words - one chunk of the scan and its
    neighbours, each with a full and with a partial last word (a word count of 4096 k + 1 also leaves the scan's last workgroup one
    count, the path that does not load 16 of them at once)."""
    rng = np.random.default_rng(nbits)
    for name, words in rank_bitmaps(nbits, rng):
        check_rank(words, nbits, (nbits, name))


def test_rank_beyond_1024_chunks_of_the_scan():
    """More than 1024 chunks of 4096 words (a bitmap of 16 MiB and a bit): every lane of the scan's second level sums more than one
    chunk.  The last word is partial."""
    nbits = 32 * F.RANK_LARGE_NWORDS - 7
    rng = np.random.default_rng(1024)
    for name, words in rank_bitmaps(nbits, rng):
        check_rank(words, nbits, ("large", name))


# ---------------------------------------------------------------------------------------------------------------- generic select + fill
def generic_column(sizes, data, words, n, invert, want, want_src, what):
    """rank, sizes(bits, rank, row, len, src), the prefix with torch, rrx_pieces_fill - through the C entries, every array of the
    caller's poisoned and exactly as long as the rule says; want = filter_rule(...), want_src = the selected rows' offsets."""
    L, s = rr._L, stream()
    rows_want, off_want, bytes_want = want
    nsel, total = len(rows_want), len(bytes_want)
    bits = dev_words(words)
    rw = L.rrx_bitmap_rank_words(n)
    rank = torch.empty(rw, dtype=torch.int64, device="cuda")
    rr._check(L.rrx_bitmap_rank(0, ptr(bits), n, invert, ptr(rank), rw, s))
    assert int(rank[(n + 31) // 32].item()) == nsel, (what, "rank total")
    row, length, src = Guarded(nsel, torch.int64), Guarded(nsel, torch.int32), Guarded(nsel, torch.int64)
    rr._check(sizes(ptr(bits), ptr(rank), row.ptr, length.ptr, src.ptr, s))
    torch.cuda.synchronize()
    assert np.array_equal(row.written((what, "d_row")), rows_want), (what, "d_row")
    lens = length.written((what, "d_piece_len")).astype(np.int64) & 0xFFFFFFFF
    assert np.array_equal(lens, np.diff(off_want)), (what, "d_piece_len", lens[:8], np.diff(off_want)[:8])
    assert np.array_equal(src.written((what, "d_piece_src")), want_src), (what, "d_piece_src")
    piece_off = torch.zeros(nsel + 1, dtype=torch.int64, device="cuda")
    if nsel:
        piece_off[1:] = torch.cumsum(length.view.to(torch.int64) & 0xFFFFFFFF, dim=0)
    out = Guarded(total, torch.uint8)
    rr._check(L.rrx_pieces_fill(0, ptr(data), src.ptr, ptr(piece_off), nsel, out.ptr, s))
    torch.cuda.synchronize()
    got = out.written((what, "d_out"))
    bad = np.nonzero(got != np.frombuffer(bytes_want, dtype=np.uint8))[0]
    assert bad.size == 0, (what, "first bad byte", int(bad[0]), "row", int(np.searchsorted(off_want, bad[0], side="right")) - 1)


def same_column(got, want, what):
    rows, off, out = got
    assert np.array_equal(rows.cpu().numpy(), want[0]) and np.array_equal(off.cpu().numpy(), want[1]) and out.cpu().numpy().tobytes() == want[2], what


# ---- items
def item_column(n, trim, first, rng):
    """n raw items of 0 .. 11 bytes of every value ('\\n', NUL and bytes >= 0x80 among them), one behind the other from offset
    `first` on -> (buffer, offsets, the items after `trim`: empty where trim exceeds the raw item)."""
    lens = rng.integers(0, 12, size=n)
    lens[rng.integers(0, 4, size=n) == 0] = 0
    off = (first + np.concatenate([[0], np.cumsum(lens)])).astype(np.int64)
    buf = rng.integers(0, 256, size=int(off[-1]) + 5, dtype=np.uint8)
    buf[rng.integers(0, 3, size=len(buf)) == 0] = 10
    raw = buf.tobytes()
    items = [raw[off[i]:max(off[i], off[i + 1] - trim)] for i in range(n)]
    return raw, off, items


@pytest.mark.parametrize("n", F.ITEM_COUNTS)
def test_items_select_and_fill(n):
    """1, 31, 32, 33, 1023, 1025 items and one more than the lanes of the bounded grid (the grid then strides); every selection;
    trim 0, 1 and 3 - more than many items have; empty items; d_off[0] = 37; items holding '\\n', NUL and bytes >= 0x80."""
    L = rr._L
    rng = np.random.default_rng(n)
    small = n <= 1025
    for trim in (0, 1, 3) if small else (1,):
        raw, off, items = item_column(n, trim, 37, rng)
        data, doff = dev_bytes(raw), torch.from_numpy(off).cuda()
        for kind in F.SELECTIONS if small else ("random", "last"):
            flags = F.selection(kind, n, rng)
            words = F.pack_bits(flags, rng)
            for invert in (0, 1):
                what = (n, "trim", trim, kind, "invert", invert)
                want = F.filter_rule(items, words, bool(invert))
                sizes = lambda b, r, row, ln, src, s: L.rrx_filter_sizes(0, ptr(doff), n, trim, b, invert, r, row, ln, src, s)
                generic_column(sizes, data, words, n, invert, want, off[want[0]], what)
            if kind == "random":
                same_column(rr.filter_rows(data, doff, dev_words(words), invert=True, trim=trim), want, (what, "filter_rows"))


def test_no_items_write_nothing():
    L, s = rr._L, stream()
    row, length, src = Guarded(0, torch.int64), Guarded(0, torch.int32), Guarded(0, torch.int64)
    rank = Guarded(L.rrx_bitmap_rank_words(0), torch.int64)
    rr._check(L.rrx_bitmap_rank(0, None, 0, 1, rank.ptr, rank.n, s))
    rr._check(L.rrx_filter_sizes(0, None, 0, 0, None, 0, rank.ptr, row.ptr, length.ptr, src.ptr, s))
    torch.cuda.synchronize()
    assert rank.written("rank")[0] == 0
    for g in (row, length, src):
        g.written("no items")
    off = torch.zeros(1, dtype=torch.int64, device="cuda")
    rows, out_off, out = rr.filter_rows(torch.empty(0, dtype=torch.uint8, device="cuda"), off, torch.empty(0, dtype=torch.int32, device="cuda"))
    assert rows.numel() == 0 and out_off.tolist() == [0] and out.numel() == 0


# ---- corpus lines
def check_corpus_case(corpus, text, extra, what, kinds=F.SELECTIONS):
    L = rr._L
    n = len(F.lines_of(text))
    assert corpus.num_lines == n, (what, corpus.num_lines, n)
    rng = np.random.default_rng(len(text))
    selections = [(kind, F.selection(kind, n, rng)) for kind in kinds] + list(extra)
    for kind, flags in selections:
        words = F.pack_bits(flags, rng)
        for invert in (0, 1):
            for keep in (0, 1):
                w = (what, kind, "invert", invert, "keep_newline", keep)
                want = F.filter_rule(text, words, bool(invert), bool(keep))
                sizes = lambda b, r, row, ln, src, s: L.rrx_filter_corpus_sizes(corpus._h, b, invert, keep, r, row, ln, src, s)
                generic_column(sizes, corpus.data, words, n, invert, want, F.sources_rule(text, words, bool(invert)), w)
    same_column(corpus.filter_lines(dev_words(words), invert=True, keep_newline=True), want, (what, "filter_lines"))
    same_column(corpus.filter_lines(dev_words(words), invert=False, keep_newline=False), F.filter_rule(text, words, False, False), (what, "filter_lines"))


@pytest.mark.parametrize("case", F.corpus_cases(), ids=lambda c: c[0])
def test_corpus_select_and_fill(case):
    """Stripes of 512 bytes.  The texts are filter_cases.corpus_cases: lines that span one, two and three stripe ends, stripes in
    which no line starts, lines that start on the last byte of a stripe, a newline as the first and as the last byte of a stripe,
    runs of empty lines, a corpus of newlines only, a final fragment without a newline (selected and not, kept newlines or not),
    data that ends 1 .. 129 bytes behind the last line start (fewer than 16, fewer than one 128-byte round), a wave of 64 stripes
    with one selected line and one with none, random texts."""
    name, text, extra = case
    check_corpus_case(rr.Corpus(dev_bytes(text), stripe=F.STRIPE), text, extra, name)


def test_corpus_select_with_the_automatic_stripe():
    """The corpus as rrx_corpus_create indexes it: the stripe is the library's choice (its line count decides; for a text of this
    size it may well be 512 bytes again - the kernel takes whatever the handle says)."""
    text = F.automatic_stripe_text()
    corpus = rr.Corpus(dev_bytes(text))
    check_corpus_case(corpus, text, [], "automatic stripe", kinds=("random", "last", "all"))


# ---------------------------------------------------------------------------------------------------------------- one-call forms
class Column:
    """The same rows three ways: an offsets column (trim 1), an indexed batch over it, and a corpus of the same bytes."""

    def __init__(self, lines):
        self.lines = list(lines)
        self.text = b"".join(ln + b"\n" for ln in self.lines)
        self.data = dev_bytes(self.text)
        off = np.concatenate([[0], np.cumsum([len(ln) + 1 for ln in self.lines])]).astype(np.int64)
        self.doff = torch.from_numpy(off).cuda()
        self.items = rr.Items(self.data, self.doff, trim=1)
        self.corpus = rr.Corpus(self.data, stripe=F.STRIPE)

    def forms(self, r, invert):
        """(name, the call on the output tail, keep_newline of the expected column)"""
        L, n = rr._L, len(self.lines)
        yield "extents", (lambda *t: L.rrx_filter_contains_extents(r._h, 0, ptr(self.data), ptr(self.doff), n, 1, invert, *t)), False
        yield "items", (lambda *t: L.rrx_filter_contains_items(r._h, self.items._h, invert, *t)), False
        yield "corpus", (lambda *t: L.rrx_filter_contains_corpus(r._h, self.corpus._h, invert, 0, *t)), False
        yield "corpus, newlines kept", (lambda *t: L.rrx_filter_contains_corpus(r._h, self.corpus._h, invert, 1, *t)), True

    def expected(self, flags, invert, keep):
        words = F.pack_bits(flags, np.random.default_rng(5))
        return F.filter_rule(self.text, words, bool(invert), keep)


def one_call(call, want, rows_cap, cap, what, null_out=False):
    """One call with the given caps: the counts are exact; d_row and d_out_off are written iff the rows fit, d_out iff the bytes
    fit too; with no row selected d_out_off[0] = 0 and nothing else."""
    rows_want, off_want, bytes_want = want
    nsel, total = len(rows_want), len(bytes_want)
    row, out_off, out = Guarded(rows_cap, torch.int64), Guarded(rows_cap + 1, torch.int64), Guarded(cap, torch.uint8)
    nrows, tot = C.c_size_t(99), C.c_size_t(99)
    rr._check(call(row.ptr, out_off.ptr, rows_cap, None if null_out else out.ptr, cap, C.byref(nrows), C.byref(tot), stream()))
    torch.cuda.synchronize()
    what = (what, "rows_cap", rows_cap, "cap", cap)
    assert (nrows.value, tot.value) == (nsel, total), (what, nrows.value, tot.value, nsel, total)
    if nsel == 0:
        assert out_off.written(what, 1)[0] == 0 and row.written(what, 0) is not None and out.written(what, 0) is not None
    elif nsel <= rows_cap:
        assert np.array_equal(row.written(what, nsel), rows_want), (what, "d_row")
        assert np.array_equal(out_off.written(what, nsel + 1), off_want), (what, "d_out_off")
        if total <= cap:
            assert out.written(what, total).tobytes() == bytes_want, (what, "d_out")
        else:
            out.written(what, 0)
    else:
        row.written(what, 0), out_off.written(what, 0), out.written(what, 0)


def cap_protocol(call, want, what):
    nsel, total = len(want[0]), len(want[2])
    one_call(call, want, nsel, total, what)
    one_call(call, want, nsel + 3, total + 5, what)
    if nsel:
        one_call(call, want, nsel - 1, total, what)
    if total:
        one_call(call, want, nsel, total - 1, what)
    one_call(call, want, nsel, 0, what, null_out=True)


@pytest.fixture(scope="module")
def column():
    return Column(F.ONE_CALL_LINES)


@pytest.mark.parametrize("pattern", F.ONE_CALL_PATTERNS)
def test_one_call_forms(column, pattern):
    """[0-9]+ and a keyword alternation on a small column, on the same bytes as an indexed batch and as a corpus, both invert
    values; caps: exact, generous, rows_cap one short, cap one short, cap == 0 with a null d_out."""
    r = rr.RRegex(pattern)
    flags = [re.search(pattern.encode(), ln) is not None for ln in column.lines]
    assert any(flags) and not all(flags)
    for invert in (0, 1):
        for name, call, keep in column.forms(r, invert):
            cap_protocol(call, column.expected(flags, invert, keep), (pattern, name, "invert", invert))
    same_column(r.filter_contains_extents(column.data, column.doff, trim=1), column.expected(flags, 0, False), "filter_contains_extents")
    same_column(r.filter_contains_items(column.items, invert=True, cap=1, rows_cap=0), column.expected(flags, 1, False), "filter_contains_items, caps grow")
    same_column(r.filter_contains_corpus(column.corpus, cap=0), column.expected(flags, 0, True), "filter_contains_corpus, cap grows")


def test_one_call_a_nullable_pattern_selects_every_row_and_the_empty_language_none(column):
    n = len(column.lines)
    for pattern, flags in (("x*", [True] * n), ("[]", [False] * n)):
        r = rr.RRegex(pattern)
        for invert in (0, 1):
            for name, call, keep in column.forms(r, invert):
                cap_protocol(call, column.expected(flags, invert, keep), (pattern, name, "invert", invert))


def test_one_call_with_zero_rows_in():
    """nitems == 0 and a corpus of zero lines: d_out_off[0] = 0, both counts 0, nothing else written - with rows_cap 0 too."""
    L = rr._L
    r = rr.RRegex("[0-9]+")
    data = dev_bytes(b"")
    doff = torch.zeros(1, dtype=torch.int64, device="cuda")
    items = rr.Items(data, doff, trim=1)
    corpus = rr.Corpus(torch.empty(0, dtype=torch.uint8, device="cuda"))
    assert corpus.num_lines == 0
    empty = (np.zeros(0, dtype=np.int64), np.zeros(1, dtype=np.int64), b"")
    for invert in (0, 1):
        for name, call in (("extents", lambda *t: L.rrx_filter_contains_extents(r._h, 0, ptr(data), ptr(doff), 0, 1, invert, *t)),
                           ("items", lambda *t: L.rrx_filter_contains_items(r._h, items._h, invert, *t)),
                           ("corpus", lambda *t: L.rrx_filter_contains_corpus(r._h, corpus._h, invert, 1, *t))):
            one_call(call, empty, 0, 0, (name, invert), null_out=True)
            one_call(call, empty, 4, 9, (name, invert))
    rows, out_off, out = r.filter_contains_corpus(corpus)
    assert rows.numel() == 0 and out_off.tolist() == [0] and out.numel() == 0
    same_column(corpus.filter_lines(torch.empty(0, dtype=torch.int32, device="cuda")), empty, "filter_lines of no lines")


def test_one_call_follows_the_contains_route(column):
    """(a|b)*a(a|b){14} has no contains table: RRX_ERR_UNSUPPORTED exactly as rrx_contains_* says it - for an empty input too -
    and the NFA route's rows under RRX_OPT_CONTAINS_NFA = 1."""
    L = rr._L
    pattern = "(a|b)*a(a|b){14}"
    lines = [b"ab" * 9, b"b" * 20, b"", b"a" + b"b" * 14, b"xx a" + b"a" * 14 + b" yy", b"a" + b"b" * 13]
    col = Column(lines)
    flags = [re.search(pattern.encode(), ln) is not None for ln in lines]
    assert flags == [True, False, False, True, True, False]
    r = rr.RRegex(pattern)
    doff0 = torch.zeros(1, dtype=torch.int64, device="cuda")
    for invert in (0, 1):
        calls = [call for _, call, _ in col.forms(r, invert)]
        calls.append(lambda *t: L.rrx_filter_contains_extents(r._h, 0, ptr(col.data), ptr(doff0), 0, 1, invert, *t))      # (no items)
        for call in calls:
            row, out_off, out = Guarded(8, torch.int64), Guarded(9, torch.int64), Guarded(64, torch.uint8)
            nrows, tot = C.c_size_t(99), C.c_size_t(99)
            assert call(row.ptr, out_off.ptr, 8, out.ptr, 64, C.byref(nrows), C.byref(tot), stream()) == ERR_UNSUPPORTED
            assert b"determinise" in L.rrx_last_error()
            torch.cuda.synchronize()
            row.written("unsupported", 0), out_off.written("unsupported", 0), out.written("unsupported", 0)
    r.set_contains_nfa(1)
    for invert in (0, 1):
        for name, call, keep in col.forms(r, invert):
            cap_protocol(call, col.expected(flags, invert, keep), (pattern, name, "invert", invert))


def test_grep_piped_into_grep(column):
    """The keep_newline = 1 output of filter_contains_corpus is a corpus again: every one of its lines contains the pattern, and
    filtering it once more returns it byte for byte; a second pattern then is grep p1 | grep p2."""
    p1, p2 = "error|warn|fatal", "[0-9]+"
    r1, r2 = rr.RRegex(p1), rr.RRegex(p2)
    rows, off, out = r1.filter_contains_corpus(column.corpus)
    first = [ln for ln in column.lines if re.search(p1.encode(), ln)]
    assert out.cpu().numpy().tobytes() == b"".join(ln + b"\n" for ln in first)
    aligned = dev_bytes(out.cpu().numpy().tobytes())               # (a corpus starts at a 16-byte aligned address)
    again = rr.Corpus(aligned, stripe=F.STRIPE)
    n = again.num_lines
    assert n == len(first)
    bits = r1.contains_corpus_bits(again).cpu().numpy().view(np.uint32)
    assert list(F.selected_rows(bits, n, False)) == list(range(n)) and rr.bitmap_count(r1.contains_corpus_bits(again), n) == n
    rows2, off2, out2 = r1.filter_contains_corpus(again)
    assert rows2.tolist() == list(range(n)) and torch.equal(off2, off) and torch.equal(out2, aligned)
    rows3, off3, out3 = r2.filter_contains_corpus(again)
    both = [ln for ln in first if re.search(p2.encode(), ln)]
    assert both and out3.cpu().numpy().tobytes() == b"".join(ln + b"\n" for ln in both)
    assert [first[i] for i in rows3.tolist()] == both
