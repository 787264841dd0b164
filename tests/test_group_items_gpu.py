"""rrx_group_spans_* / rrx_extract_group_longest_* on the device: the span of a top-level capture group inside the leftmost-longest
match of every item.  Against the brute force of the header's SEMANTICS on short items (the CPU test's patterns, items and expected
values), and on long items against answers known by construction (Python's re agrees on them and is asserted to)."""
import random
import re

import numpy as np
import pytest

import roaringregex_amd as rr
from test_group_items_lowering import GLOBAL_A, NAMED, global_items, group_brute_force, oracles_for, reference_groups
from test_search_all_longest_items_lowering import pack

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
LETTERS_DIGITS = "[a-z]*([0-9]+)-[a-z]{1,3}"        # long items by construction: A and the group as long as wanted, a C that dies at once
RUN = "[a-c]*([a-c]+)[a-c]*"                        # every offset of a run is marked: the group is the run's last byte


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"


def to_dev(text, offs):
    d = torch.from_numpy(text).cuda() if len(text) else torch.empty(0, dtype=torch.uint8, device="cuda")
    return d, torch.from_numpy(offs).cuda()


def as_array(want):
    a = np.array(want, dtype=np.int32).reshape(len(want), 2)
    a.setflags(write=False)
    return a


def assert_spans(got, want, what):
    g = torch.stack([got[0], got[1]], dim=1).cpu().numpy().astype(np.int32)
    bad = np.nonzero((g != want).any(axis=1))[0]
    assert g.shape == want.shape and bad.size == 0, (what, "first bad item", int(bad[0]), g[bad[0]].tolist(), want[bad[0]].tolist())


def run_both_forms(g, dev, doff, trim, want, what, handle=None):
    """spans after search_longest, and the fused form - on the offsets, or on an indexed batch."""
    if handle is None:
        ms, me = g.regex.search_longest_extents(dev, doff, trim=trim)
        assert_spans(g.spans_extents(dev, doff, ms, me, trim=trim), want, (what, "spans"))
        assert_spans(g.extract_extents(dev, doff, trim=trim), want, (what, "fused"))
    else:
        ms, me = g.regex.search_longest_items(handle)
        assert_spans(g.spans_items(handle, ms, me), want, (what, "indexed, spans"))
        assert_spans(g.extract_items(handle), want, (what, "indexed, fused"))


def test_short_items_against_the_brute_force():
    for p, group, items, want in reference_groups():
        g = rr.RGroup(p, group)
        want = as_array(want)
        for trim in (0, 1):
            dev, doff = to_dev(*pack(list(items), trim, lead=trim * 3, seed=len(items) + trim))
            run_both_forms(g, dev, doff, trim, want, (p, group, "trim", trim))
            run_both_forms(g, dev, doff, trim, want, (p, group, "trim", trim), handle=rr.Items(dev, doff, trim=trim))
    for p, group, item, span in NAMED:
        dev, doff = to_dev(*pack([item, b"", item], 1, lead=3))
        run_both_forms(rr.RGroup(p, group), dev, doff, 1, as_array([span, group_brute_force(p, group, b""), span]), (p, group, "named case"))


POOL = [b"", b"a", b"12-345", b"x 12-345 y", b"-", b"1-", b"007-1-22", b"ab;;", b"zzzzzzzzzzzzzzzz9-0", b"5-5\x00\xff", b"12 - 3"]


def pooled_batch(n, seed, lead):
    """n items drawn from POOL, each followed by one separator byte, `lead` bytes in front; built with numpy -> (text, offsets, index)."""
    rng = np.random.default_rng(seed)
    regions = [it + b";" for it in POOL]
    flat = np.frombuffer(b"".join(regions), dtype=np.uint8)
    rlen = np.array([len(x) for x in regions], dtype=np.int64)
    roff = np.concatenate([[0], np.cumsum(rlen)[:-1]])
    idx = rng.integers(0, len(POOL), size=n)
    lens = rlen[idx]
    off = np.concatenate([[0], np.cumsum(lens)])
    src = np.arange(int(off[-1]), dtype=np.int64) - np.repeat(off[:-1], lens) + np.repeat(roff[idx], lens)
    text = np.concatenate([np.full(lead, ord("q"), dtype=np.uint8), flat[src]])
    return text, off + lead, idx


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, 65536 + 65])
def test_batch_sizes(n):
    """Wave edges (63, 64, 65), more than one workgroup (4097: five) and 65 workgroups; the offsets do not begin at 0."""
    text, off, idx = pooled_batch(n, 50 + n % 7, lead=16)
    dev, doff = to_dev(text, off)
    assert dev.untyped_storage().nbytes() == int(off[-1])           # the text tensor ends with the last item
    for group in (1, 2):
        per = as_array([group_brute_force("([0-9]+)-([0-9]+)", group, it) for it in POOL])
        assert 2 < int((per[:, 0] >= 0).sum()) < len(POOL)
        run_both_forms(rr.RGroup("([0-9]+)-([0-9]+)", group), dev, doff, 1, per[idx], ("batch", n, group))


def constructed(p, lead, letters, digits, tail):
    """One item for LETTERS_DIGITS and where its group is: junk, `letters` of [a-z], `digits` of [0-9], '-', the tail."""
    it = b" ;" * lead + b"kq" * (letters // 2) + b"w" * (letters % 2) + b"7" * digits + b"-" + tail
    at = 2 * lead + letters
    return it, ((at, at + digits) if digits and tail[:1].isalpha() else (-1, -1))


def test_every_alignment_of_item_start_and_mark_word():
    """Items of 0 ... 100 bytes, each 32 times in a row at an odd pitch: (b - base) mod 32 takes all 32 residues and the byte address
    all 16; then the whole buffer off 16-byte alignment."""
    shapes = [(b"", (-1, -1)), (b"a", (-1, -1))]
    for letters, digits in ((0, 1), (3, 27), (10, 21), (29, 3), (31, 31), (40, 23), (1, 62), (64, 33)):
        shapes.append(constructed(LETTERS_DIGITS, 0, letters, digits, b"ab"))
    shapes.append((b"x" * 3 + b"abcabcbacb" * 9 + b"xx", (92, 93)))                       # RUN
    for p, group, chosen in ((LETTERS_DIGITS, 1, shapes[:-1]), (RUN, 1, shapes[:2] + shapes[-1:])):
        for it, span in chosen:
            m = re.search(p.encode(), it)
            assert (m.span(1) if m else (-1, -1)) == span or p == RUN, (p, it)
        items, want = [], []
        for it, span in chosen:
            for _ in range(32):
                items += [it] if len(it) % 2 == 0 else [it, b""]    # pitch = item + separator (+ an empty item's separator): odd
                want += [span] if len(it) % 2 == 0 else [span, (-1, -1)]
        if p == RUN:
            want = [(-1, -1) if not it else ((0, 1) if it == b"a" else w) for it, w in zip(items, want)]
            assert group_brute_force(RUN, 1, b"xxabcabcbxx") == (8, 9)
        g = rr.RGroup(p, group)
        for lead in (0, 3):
            text, offs = pack(items, 1, lead)
            base = int(offs[0])
            for it, _ in chosen:
                at = [int(o) for o, x in zip(offs[:-1], items) if x == it]
                assert len({(o - base) % 32 for o in at}) == 32 and len({o % 16 for o in at}) == 16, (len(it), lead)
            dev, doff = to_dev(text, offs)
            run_both_forms(g, dev, doff, 1, as_array(want), (p, "alignment", lead))
            run_both_forms(g, dev, doff, 1, as_array(want), (p, "alignment, indexed", lead), handle=rr.Items(dev, doff, trim=1))
            sliced = torch.cat([torch.zeros(5, dtype=torch.uint8, device="cuda"), dev])[5:]
            assert sliced.data_ptr() % 16 == 5
            run_both_forms(g, sliced, doff, 1, as_array(want), (p, "alignment, sliced", lead))


def test_long_items():
    """5 KB ... 135 KB per item: a 60 KB A, a 30 KB group, a C on which the reverse table dies after four bytes (the marks of the
    30 KB in front of it are zero words written without the text), a run of 40 KB every offset of which is marked, items without a
    match - on the LDS tables and with the tables forced into HBM/L2."""
    junk = b"ab12 " * 1000                                          # (no '-': nothing matches inside it)
    built = [constructed(LETTERS_DIGITS, 5, 60000, 40, b"abc;" + junk), constructed(LETTERS_DIGITS, 0, 100, 30000, b"xy"),
             constructed(LETTERS_DIGITS, 2500, 5000, 5000, b"abcd"), (junk, (-1, -1)), constructed(LETTERS_DIGITS, 9, 70000, 60000, b"#a"),
             constructed(LETTERS_DIGITS, 1, 4999, 1, b"q" + junk)]
    for it, span in built:
        assert 5000 <= len(it) <= 135000
        if span[0] >= 0:                                            # (Python's search backtracks quadratically on the items without a match)
            assert re.search(LETTERS_DIGITS.encode(), it).span(1) == span
        else:
            assert not re.search(rb"[0-9]-[a-z]", it)
    assert max(e - s for _, (s, e) in built) == 30000 and sum(s < 0 for _, (s, _) in built) == 2
    runs = [(b"x" * 700 + b"abc" * 13334 + b"xx", (700 + 40001, 700 + 40002)), (b"xyz" * 2000, (-1, -1)), (b"c" * 5000, (4999, 5000))]
    for p, cases in ((LETTERS_DIGITS, built), (RUN, runs)):
        items, want = [it for it, _ in cases], as_array([span for _, span in cases])
        for engine in (rr.ENGINE_AUTO, rr.ENGINE_DFA_GLOBAL):
            g = rr.RGroup(p, 1, engine)
            for trim, lead in ((0, 0), (1, 7)):
                dev, doff = to_dev(*pack(items, trim, lead, seed=trim))
                run_both_forms(g, dev, doff, trim, want, (p, "long", engine, trim))


def test_both_table_placements():
    """RRX_ENGINE_DFA_GLOBAL forces every table into HBM/L2; under AUTO a part whose tables pass 64 KiB goes there on its own."""
    for p, group, items, want in reference_groups()[:8]:
        dev, doff = to_dev(*pack(list(items), 1, lead=2))
        run_both_forms(rr.RGroup(p, group, rr.ENGINE_DFA_GLOBAL), dev, doff, 1, as_array(want), (p, group, "global form"))
    g = rr.RGroup(GLOBAL_A, 1)
    a, rev = g.program(rr.PROGRAM_GROUP_A), g.program(rr.PROGRAM_GROUP_REV_BC)
    assert int(a[0]) * int(a[1]) * 2 + int(rev[0]) * int(rev[1]) * 2 > 65536
    items, want = global_items(random.Random(61), 300, 64)
    assert 20 < sum(w[0] >= 0 for w in want) < len(items) - 20
    for trim, lead in ((0, 0), (1, 9)):
        dev, doff = to_dev(*pack(items, trim, lead))
        run_both_forms(g, dev, doff, trim, as_array(want), ("AUTO, tables beyond the LDS budget", trim))


def filled(n, byte, dtype=torch.int32):
    return torch.full((n,), byte * 0x01010101 - (1 << 32 if byte >= 0x80 else 0), dtype=dtype, device="cuda")


def test_poisoned_buffers_and_the_end_of_the_marks():
    """Marks, both result arrays and the gaps between items poisoned with 0xFF (and, to see every result word written, with 0x5A);
    the bytes of d_marks at and beyond marks_words stay as they were - also when marks_words is too small for the batch."""
    p, group, items, want = next(x for x in reference_groups() if x[0] == "[ab]*(a[ab]*)b[ab]*")
    items, n = list(items), len(items)
    want = as_array(want)
    offs = np.zeros(n + 1, dtype=np.int64)
    parts, at = [b"\xff" * 5], 5
    offs[0] = at
    for k, it in enumerate(items):
        parts.append(it + b"\xff" * 3)                               # trim 3: three bytes of 0xFF behind every item
        at += len(it) + 3
        offs[k + 1] = at
    text = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
    dev, doff = to_dev(text, offs)
    g = rr.RGroup(p, group)
    L, s = rr._L, rr._stream_ptr(None)
    words = L.rrx_search_all_longest_marks_words(int(offs[-1] - offs[0]), n)
    for byte in (0xFF, 0x5A):
        for short_by in (0, words - (n + 1)):                       # the whole buffer; the smallest the entry takes
            given = words - short_by
            marks, gs, ge = filled(words + 8, byte), filled(n + 1, byte), filled(n + 1, byte)
            rr._check(L.rrx_extract_group_longest_extents(g._h, 0, dev.data_ptr(), doff.data_ptr(), n, 3, marks.data_ptr(), given, gs.data_ptr(), ge.data_ptr(), s))
            torch.cuda.synchronize()
            assert bool((marks[given:] == filled(1, byte)).all()), (byte, short_by, "a mark word at or beyond marks_words was written")
            assert bool(gs[n] == filled(1, byte)[0]) and bool(ge[n] == filled(1, byte)[0])
            if not short_by:
                assert_spans((gs[:n], ge[:n]), want, ("poison", byte))
            if byte == 0x5A:
                assert bool((gs[:n] != POISON).all()) and bool((ge[:n] != POISON).all()), "a result word was not written"
    assert L.rrx_extract_group_longest_extents(g._h, 0, dev.data_ptr(), doff.data_ptr(), n, 3, marks.data_ptr(), n, gs.data_ptr(), ge.data_ptr(), s) == 2
    # both A and C absent: no launch, d_marks may be null
    bare = rr.RGroup("(a[ab]*)", 1)
    gs, ge = filled(n, 0x5A), filled(n, 0x5A)
    rr._check(L.rrx_extract_group_longest_extents(bare._h, 0, dev.data_ptr(), doff.data_ptr(), n, 3, None, 0, gs.data_ptr(), ge.data_ptr(), s))
    ms, me = bare.regex.search_longest_extents(dev, doff, trim=3)
    assert torch.equal(gs, ms) and torch.equal(ge, me) and int((ms >= 0).sum()) > 10
    # the empty language: two fills
    none = rr.RGroup("a([])b", 1)
    assert_spans(none.extract_extents(dev, doff, trim=3), as_array([(-1, -1)] * n), "empty language")
    # an empty batch writes nothing
    zero = torch.zeros(1, dtype=torch.int64, device="cuda")
    st, en = g.extract_extents(torch.empty(0, dtype=torch.uint8, device="cuda"), zero)
    assert st.numel() == 0 and en.numel() == 0


def test_in_place_and_spans_that_are_no_matches():
    p, group, items, want = next(x for x in reference_groups() if x[0] == "[a-z]*([0-9]+)[0-9]")
    more = [b"ab10", b"12", b"199", b"a1"]
    items = list(items) + more
    want = as_array(list(want) + [group_brute_force(p, group, it) for it in more])
    g = rr.RGroup(p, group)
    dev, doff = to_dev(*pack(items, 1, lead=4))
    handle = rr.Items(dev, doff, trim=1)
    ms, me = g.regex.search_longest_extents(dev, doff, trim=1)
    keep_s, keep_e = ms.clone(), me.clone()
    assert_spans(g.spans_extents(dev, doff, ms, me, trim=1), want, "separate arrays")
    assert torch.equal(ms, keep_s) and torch.equal(me, keep_e), "the input list was written"
    out = g.spans_extents(dev, doff, ms, me, trim=1, out=(ms, me))                        # in place
    assert out[0] is ms and out[1] is me
    assert_spans((ms, me), want, "in place")
    ms, me = keep_s.clone(), keep_e.clone()
    g.spans_items(handle, ms, me, out=(ms, me))
    assert_spans((ms, me), want, "in place, indexed")
    # only one of the two in place; the other group of a pattern whose A is absent
    ms = keep_s.clone()
    assert_spans(g.spans_extents(dev, doff, ms, keep_e, trim=1, out=(ms, torch.empty_like(ms))), want, "start in place")
    # spans that are no matches: every item's whole extent, and every match cut short by one byte
    lens = torch.tensor([len(it) for it in items], dtype=torch.int32, device="cuda")
    whole_s, whole_e = torch.zeros_like(lens), lens.clone()
    got = g.spans_extents(dev, doff, whole_s, whole_e, trim=1)
    # (the whole item is a match of P exactly where P accepts it: elsewhere the list is no match and none is reported)
    accepts_whole = np.array([oracles_for(p, group)[0].accepts(it) for it in items])
    assert 2 < int(accepts_whole.sum()) < len(items) // 2
    assert np.array_equal(got[0].cpu().numpy() >= 0, accepts_whole) and np.array_equal(got[1].cpu().numpy() >= 0, accepts_whole)
    assert_spans((got[0][-4:], got[1][-4:]), want[-4:], "the whole item where it is the match")
    wild_s, wild_e = torch.full_like(lens, 0x7FFFFFF0), torch.full_like(lens, -2)          # beyond every item: clamped, nothing outside is read
    got = g.spans_extents(dev, doff, wild_s, wild_e, trim=1)
    assert bool((got[0] == -1).all()) and bool((got[1] == -1).all())


def test_a_side_stream_and_a_captured_graph():
    p, group, items, want = next(x for x in reference_groups() if x[0] == "[a-c]*([a-c]+)[a-c]*")
    items, n = list(items), len(items)
    g = rr.RGroup(p, group)
    text, offs = pack(items, 1, lead=1)
    dev, doff = to_dev(text, offs)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    got = g.extract_extents(dev, doff, trim=1, stream=side)         # (eager, the warm-up: the tables are uploaded here)
    ms, me = g.regex.search_longest_extents(dev, doff, trim=1, stream=side)
    got2 = g.spans_extents(dev, doff, ms, me, trim=1, stream=side)
    side.synchronize()
    assert_spans(got, as_array(want), "side stream, fused")
    assert_spans(got2, as_array(want), "side stream, spans")
    # the fused form captured once (nothing is allocated, uploaded or read back inside it), replayed on refilled inputs
    words = rr._L.rrx_search_all_longest_marks_words(len(text), n)
    marks = torch.full((words,), POISON, dtype=torch.int32, device="cuda")
    gs, ge = torch.full((n,), POISON, dtype=torch.int32, device="cuda"), torch.full((n,), POISON, dtype=torch.int32, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            g.extract_extents(dev, doff, trim=1, out=(gs, ge), marks=marks, stream=side)
    torch.cuda.current_stream().wait_stream(side)
    for round_, order in enumerate((list(range(n)), list(reversed(range(n))))):
        text2, offs2 = pack([items[k] for k in order], 1, lead=1)
        assert len(text2) == len(text)
        dev.copy_(torch.from_numpy(text2))
        doff.copy_(torch.from_numpy(offs2))
        for t in (marks, gs, ge):
            t.fill_(POISON)
        graph.replay()
        torch.cuda.synchronize()
        assert_spans((gs, ge), as_array([want[k] for k in order]), ("replay", round_))


def test_extract_column():
    for p, group, items, want in reference_groups()[:6]:
        items = list(items)
        g = rr.RGroup(p, group)
        for trim in (0, 1):
            dev, doff = to_dev(*pack(items, trim, lead=2))
            valid, out_off, out = g.extract_column(dev, doff, trim=trim)
            off, buf = out_off.cpu().numpy(), out.cpu().numpy().tobytes()
            assert valid.cpu().numpy().tolist() == [s >= 0 for s, _ in want] and off[0] == 0 and off[-1] == len(buf)
            got = [buf[off[k]:off[k + 1]] for k in range(len(items))]
            assert got == [it[s:e] if s >= 0 else b"" for it, (s, e) in zip(items, want)], (p, group, trim)
    g = rr.RGroup("https?://([^/]+)/.*", 1)
    dev, doff = to_dev(*pack([b"see http://example.com/a/b", b"no url", b"https://h/"], 1))
    valid, out_off, out = g.extract_column(dev, doff, trim=1)
    assert valid.tolist() == [True, False, True] and out.cpu().numpy().tobytes() == b"example.comh" and out_off.tolist() == [0, 11, 11, 12]
