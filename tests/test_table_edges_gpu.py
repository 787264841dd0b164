"""The automata on the limit of every table form (table_edge_cases.py) on the device: every case on every entry that reads its
table, each result compared bit for bit with the expected verdicts, every output written over a dirty buffer with guard words
behind it.  An off-by-one in a fit rule or in a kernel's address arithmetic (a shift by rep_log2, a signed 16-bit read, a base
added to an offset beyond 32 KiB) gives wrong transitions only in the last rows of such an automaton; the texts walk those rows
(test_table_edges_lowering.py shows that they would notice).

The one-call items entry (match_extents) goes stripe-wise only from 65536 items and 8 MiB on; the texts here stay below 1 MiB, so it
runs a lane per item here, and the two items tables are read through match_items on an indexed batch, with the stride-2 items
form on and off."""
import re

import numpy as np
import pytest

import roaringregex_amd as rr
import table_edge_cases as T
from contains_cases import unpack
from pyoracle import OracleRegex

torch = pytest.importorskip("torch")
from dirty_bitmap import FILLS, run_dirty, words_of  # noqa: E402  (it imports torch)

pytestmark = pytest.mark.gpu

SEPARATORS = b"\nab;\x00\xff"               # what follows an item is skipped whatever its value


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"


def ids(table):
    return [c.id for c in T.cases(table)]


def regex_of(case):
    r = rr.RRegex(case.pattern, case.engine)
    r.set_background_order(False)
    return r


def corpus_at(dev, stripe):
    corpus = rr.Corpus(dev, stripe=stripe)
    if stripe:
        assert corpus.stripe == stripe and (corpus.num_bytes + stripe - 1) // stripe > (T.WG_STRIPES if stripe == 512 else 0)
    return corpus


def dirty_bytes(call, n, want, what):
    """call(out=) writes one byte per line / item into a dirty buffer: n bytes as expected, the 16 bytes behind them untouched."""
    out = torch.full((n + 16,), 0xAA, dtype=torch.uint8, device="cuda")
    got = call(out=out)
    assert got.numel() == n
    host = out.cpu().numpy()
    bad = np.nonzero(host[:n] != want)[0]
    assert bad.size == 0, (what, "first bad", int(bad[0]), "of", n, int(host[bad[0]]))
    assert (host[n:] == 0xAA).all(), (what, "bytes behind the output were written")


def as_items(distinct, idx):
    """The lines as explicit items with one separator byte each (trim 1) -> (device bytes, device offsets)."""
    parts = [distinct[i] + SEPARATORS[k % len(SEPARATORS):k % len(SEPARATORS) + 1] for k, i in enumerate(idx)]
    offs = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    text = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
    return torch.from_numpy(text).cuda(), torch.from_numpy(offs).cuda()


# ------------------------------------------------------------------------------------------------------------ match tables
@pytest.mark.parametrize("case_id", ids("match"))
def test_match_table(case_id):
    case = T.BY_ID[case_id]
    data, want = T.expected(case_id)
    clean, want_clean = T.expected(case_id, False)
    distinct, idx = T.build_lines(case_id)
    r = regex_of(case)
    assert r.engine_name == case.form, (case_id, r.engine_name)
    dev, dev_clean = torch.from_numpy(data).cuda(), torch.from_numpy(clean).cuda()
    n = len(want)
    # rrx_match_corpus: stripe 512 (more than one workgroup, a member across the cut) and the automatic stripe; with bytes >= 0x80
    # in the text and without (the two builds of the kernels)
    c512 = corpus_at(dev, 512)
    run_dirty(r.match_corpus_bits, c512, want, fill=FILLS[0], what=(case_id, "stripe 512"))
    run_dirty(r.match_corpus_bits, corpus_at(dev, 0), want, fill=FILLS[1], what=(case_id, "automatic stripe"))
    run_dirty(r.match_corpus_bits, corpus_at(dev_clean, 512), want_clean, fill=FILLS[2], what=(case_id, "stripe 512, no high bytes"))
    run_dirty(r.match_corpus_bits, corpus_at(dev_clean, 0), want_clean, fill=FILLS[3], what=(case_id, "automatic stripe, no high bytes"))
    # rrx_match_device: the one-pass entry, over a dirty bitmap sized for a line per byte
    for text, expect, what in ((dev, want, "high bytes"), (dev_clean, want_clean, "no high bytes")):
        cap = (text.numel() + 1 + 31) // 32
        out = torch.full((cap + 8,), FILLS[1], dtype=torch.int32, device="cuda")
        bits, nlines = r.match_device_bits(text, out=out)
        assert nlines == len(expect), (case_id, what, nlines)
        host = out.cpu().numpy().view(np.uint32)
        ref = words_of(expect, (len(expect) + 31) // 32)
        bad = np.nonzero(host[:len(ref)] != ref)[0]
        assert bad.size == 0, (case_id, "match_device_bits", what, "word", int(bad[0]), hex(int(host[bad[0]])), hex(int(ref[bad[0]])))
        assert (host[cap:] == np.uint32(FILLS[1])).all(), (case_id, what, "words behind the bitmap were written")
    # rrx_match_corpus + rrx_bitmap_to_bytes
    dirty_bytes(lambda out: r.match_corpus(c512, out=out), n, want, (case_id, "match_corpus"))
    # the reference's interface on three of the edge lines: the member, one byte short, one byte long
    m, per_line = case.members[0], T.closed_form(case, distinct)
    for ln in (m, m[:-1], m + m[-1:]):
        v = r.get_acceptance_iter(ln).advance().value()
        assert (v is not None) == bool(per_line[distinct.index(ln)]), (case_id, "get_acceptance_iter", len(ln))
    # the stride-2 table in an order profiled on a sample of the case's own text: the bits stay.  Half-wave-like samples (64 lanes of
    # 4 KiB) move another row to the highest offset for a{1534} and a{1,1534}, the 256 x 256 sample for the double literal; the
    # search leaves the last row of (ab|cd|ef){127} in place with every sample shape, and permutes 60 others.
    if case.form == "dfa-stride2-table":
        lanes, per = (256, 256) if case_id == "stride2-alnum-x2" else (64, 4096)
        ordered = regex_of(case)
        order = ordered.order_table(np.ascontiguousarray(data[:lanes * per].reshape(lanes, per)), lanes, per)
        assert order is not None, case_id
        w = ordered.program(rr.PROGRAM_DFA2_ORDER)
        rows = w[2:2 + int(w[0])]
        assert int((rows != np.arange(len(rows))).sum()) >= 10, (case_id, "rows moved")
        assert (int(np.argmax(rows)) != len(rows) - 1) == (case_id != "stride2-alt{127}"), (case_id, "the row at the highest offset", int(np.argmax(rows)))
        run_dirty(ordered.match_corpus_bits, c512, want, fill=FILLS[2], what=(case_id, "ordered table"))
        run_dirty(ordered.match_corpus_bits, corpus_at(dev_clean, 512), want_clean, fill=FILLS[3], what=(case_id, "ordered table, no high bytes"))


def test_more_result_words_than_the_window_of_the_largest_table():
    """a{1,1534} leaves the smallest result window there is, 1024 words; lines of 1 to 3 bytes end more than 32768 lines per
    workgroup at stripe 512.  The corpus reports its span, the launch takes the path that clears the bitmap, and every bit is right
    - at stripe 2048 (four times the lines per workgroup) too."""
    case = T.BY_ID["stride2-a{1,1534}"]
    data, want = T.window_overflow_text()
    o = OracleRegex(case.pattern)
    for ln in (b"a", b"b", b"aa", b"ab", b"ba", b"aaa", b"aab", b"baa", b"bbb"):
        assert int(o.match_lines(np.frombuffer(ln + b"\n", dtype=np.uint8))[0]) == (1 if set(ln) == {ord("a")} else 0)
    assert 0.2 < want.mean() < 0.6
    r = regex_of(case)
    d2 = r.program(rr.ENGINE_DFA2)
    assert r.engine_name == case.form and T.dfa2_bytes(d2) == T.DFA2_MAX_TABLE
    assert (46 * 1024 - T.dfa2_bytes(d2)) // 4 == T.DFA2_WINDOW_WORDS_AT_LIMIT
    dev = torch.from_numpy(data).cuda()
    for k, stripe in enumerate((512, 2048)):
        corpus = corpus_at(dev, stripe)
        lines_per_wg = int((data[:T.WG_STRIPES * stripe] == 10).sum())
        assert lines_per_wg // 32 > T.DFA2_WINDOW_WORDS_AT_LIMIT
        # no bitmap word lies in three workgroups' ranges, but a workgroup's words pass the window
        assert corpus.one_launch and corpus.one_launch_span > T.DFA2_WINDOW_WORDS_AT_LIMIT, (stripe, corpus.one_launch_span)
        assert abs(corpus.one_launch_span - lines_per_wg // 32) <= lines_per_wg // 320, (stripe, corpus.one_launch_span, lines_per_wg // 32)
        run_dirty(r.match_corpus_bits, corpus, want, fill=FILLS[k], what=("window", stripe))
        run_dirty(r.match_corpus_bits, corpus, want, fill=FILLS[k + 2], what=("window, second launch", stripe))


# ------------------------------------------------------------------------------------------------------------ contains tables
@pytest.mark.parametrize("case_id", ids("contains"))
def test_contains_table(case_id):
    case = T.BY_ID[case_id]
    r = regex_of(case)
    assert r.contains_engine_name == case.form, (case_id, r.contains_engine_name)
    for k, high in enumerate((True, False)):                  # (the kernel that steps bytes >= 0x80 as 0x00, and the one for clean text)
        data, want = T.expected(case_id, high)
        assert bool((data >= 0x80).any()) == high
        dev = torch.from_numpy(data).cuda()
        run_dirty(r.contains_corpus_bits, corpus_at(dev, 512), want, fill=FILLS[k], what=(case_id, "stripe 512", high))
        run_dirty(r.contains_corpus_bits, corpus_at(dev, 0), want, fill=FILLS[k + 2], what=(case_id, "automatic stripe", high))


# ------------------------------------------------------------------------------------------------------------ items tables
# the path of an indexed batch with the stride-2 items form on / off (items.cpp: pick_items_table)
ITEMS_PATHS = {
    "items-a{123}": ("stride-2 items table", "byte-stride items table"),        # 125 states: the last byte-stride items table
    "items-past-a{124}": ("stride-2 items table", "lane per item"),             # 126 states: it no longer packs
    "items2-a{1534}": ("stride-2 items table", "lane per item"),                # the last stride-2 items table
    "items2-past-a{1535}": ("lane per item", "lane per item"),
}
@pytest.mark.parametrize("case_id", ids("items"))
def test_items_table(case_id):
    case = T.BY_ID[case_id]
    data, want = T.expected(case_id)
    distinct, idx = T.build_lines(case_id)
    dev, doff = as_items(distinct, idx)
    n = len(idx)
    handle = rr.Items(dev, doff, trim=1)
    assert handle.num_items == n and handle.stripe_wise
    D = int(rr.RRegex(case.pattern).program(rr.ENGINE_DFA)[0])
    packs = D * 131 * 4 * T.items_copies(D) <= 65535
    for stride2 in (True, False):
        r = regex_of(case)
        r.set_items_stride2(stride2)
        has2 = r.program(rr.PROGRAM_DFA2_ITEMS) is not None
        # the path: the stride-2 items table, else the byte-stride one where it packs, else a lane per item on the plain table
        path = "stride-2 items table" if has2 and stride2 else "byte-stride items table" if packs else "lane per item"
        assert path == ITEMS_PATHS[case_id][0 if stride2 else 1] and case.form in ITEMS_PATHS[case_id], (case_id, stride2, path)
        dirty_bytes(lambda out: r.match_items(handle, out=out), n, want, (case_id, "match_items", path))
        dirty_bytes(lambda out: r.match_extents(dev, doff, trim=1, out=out), n, want, (case_id, "match_extents", stride2))


# ------------------------------------------------------------------------------------------------------------ plain tables
def item_batch(case_id):
    """The case's lines as a small batch of items (a lane per item: far below the stripe-wise thresholds)."""
    case = T.BY_ID[case_id]
    distinct, idx = T.build_lines(case_id, True, 3 * sum(len(ln) + 1 for ln in T.distinct_lines(case)))
    assert len(idx) < 65536
    return case, distinct, idx, as_items(distinct, idx)


@pytest.mark.parametrize("case_id", ids("plain"))
def test_single_plain_table(case_id):
    """match_extents and contains_extents on a plain table of exactly the LDS budget, and on the first one that stays in HBM/L2."""
    case, distinct, idx, (dev, doff) = item_batch(case_id)
    r = regex_of(case)
    table = r.program(rr.ENGINE_DFA)
    assert (T.plain_lds_bytes(table) <= T.PLAIN_LDS_BUDGET) == (case.form == "lds") and T.plain_lds_bytes(table) == case.value
    data, want = T.expected(case_id, True, 3 * sum(len(ln) + 1 for ln in T.distinct_lines(case)))
    assert 0 < want.sum() < len(want)
    dirty_bytes(lambda out: r.match_extents(dev, doff, trim=1, out=out), len(idx), want, (case_id, "match_extents"))
    contains = r.program(rr.PROGRAM_CONTAINS_DFA)
    if contains is None:
        return                                                 # (a{13054}: no contains table)
    assert T.plain_lds_bytes(contains) == case.value
    per_line = T.contains_expected(case, distinct)
    want_c = per_line[idx]
    assert want.sum() < want_c.sum() < len(want_c)
    dirty_bytes(lambda out: r.contains_extents(dev, doff, trim=1, out=out), len(idx), want_c, (case_id, "contains_extents"))
    bits = r.contains_extents_bits(dev, doff, trim=1)
    assert (unpack(bits.cpu().numpy(), len(idx)) == want_c).all(), (case_id, "contains_extents_bits")


@pytest.mark.parametrize("case_id", ids("plain2"))
def test_two_plain_tables_of_the_leftmost_longest_search(case_id):
    """search_longest_extents on two tables that together take exactly the LDS budget, and on the first pair that does not.  The
    brute force of the search tests is cubic in the item length; on items of 6.5 KB the expected spans come from Python's re
    (a{n}: the leftmost match is the longest), and the oracle confirms every span it names and every item without one."""
    case, distinct, idx, (dev, doff) = item_batch(case_id)
    r = regex_of(case)
    st, an = r.program(rr.PROGRAM_SEARCH_STARTS), r.program(rr.PROGRAM_SEARCH_ANCHORED)
    size = T.plain_lds_bytes(st) + T.plain_lds_bytes(an)
    assert size == case.value and (size <= T.PLAIN_LDS_BUDGET) == (case.form == "lds")
    rx = re.compile(case.pattern.encode())
    o, o_any = OracleRegex(case.pattern), OracleRegex(".*(" + case.pattern + ").*")
    spans = []
    for ln in distinct:
        m = rx.search(ln)
        spans.append((m.start(), m.end()) if m else (-1, -1))
        if m:
            assert o.accepts(ln[m.start():m.end()].decode("latin-1")) and not rx.search(ln[:m.end() - 1])
        elif not any(c == 0 or c >= 0x80 for c in ln):
            assert not o_any.accepts(ln.decode("latin-1"))
    want = np.array(spans, dtype=np.int32)[idx]
    assert 0 < (want[:, 0] >= 0).sum() < len(want) and (want[:, 0] > 0).any()
    start, end = r.search_longest_extents(dev, doff, trim=1)
    got = np.stack([start.cpu().numpy(), end.cpu().numpy()], axis=1)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (case_id, "item", int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())
