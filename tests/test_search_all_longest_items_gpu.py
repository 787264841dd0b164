"""rrx_search_all_longest_extents* / rrx_search_all_longest_items* on the device: every leftmost-longest match of every item, match
k + 1 searched in the rest of the item behind match k.  Against the oracle's iterated brute force on short items (the CPU test's
patterns, items and expected values), re.finditer on patterns for which its greedy search names the same list
(test_search_all_longest_items_lowering checks that), and on large text the CPU replay of the two tables and the marks plus the
invariants that tie the answer to rrx_search_longest_extents' and rrx_search_all_extents_count's."""
import ctypes as C
import random
import re

import numpy as np
import pytest

import roaringregex_amd as rr
from contains_cases import EXPLODING
from patterns import EMAIL, K1000_CONTAINS, U2
from test_contains_items_lowering import NEWLINE_PATTERNS, short_items
from table_edge_cases import plain_table_bytes
from test_search_longest_items_lowering import GLOBAL_AUTO, global_auto_items
from test_search_all_longest_items_lowering import SearchAllLongestReplay, finditer_all, pack, reference_all, want_for

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
MAX_BLOCKS_ITEMS = 1024 * 1024                      # kernels_search_all_longest_items.hip: 1024 workgroups of 1024 lanes, then the grid strides


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"


def to_dev(text, offs):
    d = torch.from_numpy(text).cuda() if len(text) else torch.empty(0, dtype=torch.uint8, device="cuda")
    return d, torch.from_numpy(offs).cuda()


def csr(want):
    """[[(start, end)]] per item -> (count[n] int32, first[n + 1] int64, pairs[total, 2] int32), read-only."""
    count = np.array([len(w) for w in want], dtype=np.int32)
    first = np.concatenate([[0], np.cumsum(count, dtype=np.int64)]).astype(np.int64)
    pairs = np.array([x for w in want for x in w], dtype=np.int32).reshape(-1, 2)
    for a in (count, first, pairs):
        a.setflags(write=False)
    return count, first, pairs


def assert_csr(got, want, what):
    """got: (count or None, first, start, end) device tensors; first has n entries (two passes) or n + 1 (one call)."""
    count, first, pairs = want
    g_count, g_first, g_start, g_end = got
    n, total = len(count), len(pairs)
    if g_count is not None:
        gc = g_count.cpu().numpy()
        bad = np.nonzero(gc != count)[0]
        assert bad.size == 0, (what, "count, first bad item", int(bad[0]), int(gc[bad[0]]), int(count[bad[0]]))
        assert g_first.numel() == n
    else:
        assert g_first.numel() == n + 1 and int(g_first[-1]) == total, (what, "first[-1] is the total", int(g_first[-1]), total)
    assert np.array_equal(g_first.cpu().numpy(), first[:g_first.numel()]), (what, "first")
    assert g_start.numel() == total and g_end.numel() == total, (what, g_start.numel(), total)
    got_pairs = torch.stack([g_start, g_end], dim=1).cpu().numpy()
    bad = np.nonzero((got_pairs != pairs).any(axis=1))[0]
    assert bad.size == 0, (what, "first bad slot", int(bad[0]), "item", int(np.searchsorted(first, bad[0], side="right")) - 1,
                           got_pairs[bad[0]].tolist(), pairs[bad[0]].tolist())


def run_all_forms(r, dev, doff, trim, want, what, handle=None, caps=(None, 1)):
    """count + fill, then the one-call form at every cap - on the offsets, or on an indexed batch."""
    if handle is None:
        assert_csr(r.search_all_longest_extents(dev, doff, trim=trim), want, (what, "two passes"))
        for cap in caps:
            assert_csr((None,) + r.search_all_longest_extents_fused(dev, doff, trim=trim, cap=cap), want, (what, "one call, cap", cap))
    else:
        assert_csr(r.search_all_longest_items(handle), want, (what, "indexed, two passes"))
        for cap in caps:
            assert_csr((None,) + r.search_all_longest_items_fused(handle, cap=cap), want, (what, "indexed, one call, cap", cap))


def test_short_items_against_the_brute_force():
    for p, items, want_lists in reference_all():
        r = rr.RRegex(p)
        want = csr(want_lists)
        for trim in (0, 1):
            dev, doff = to_dev(*pack(items, trim, lead=trim * 3, seed=len(items) + trim))
            run_all_forms(r, dev, doff, trim, want, (p[:30], "trim", trim))
            run_all_forms(r, dev, doff, trim, want, (p[:30], "trim", trim), handle=rr.Items(dev, doff, trim=trim))
    for p, item in (("abcd|c", b"cabcdc"), ("ab|b+", b"abbbab"), ("[0-9]+", b"a1 22 333"), ("a*", b"baab")):
        dev, doff = to_dev(*pack([item] * 3, 1, lead=3))
        run_all_forms(rr.RRegex(p), dev, doff, 1, csr(want_for(p, [item] * 3)), (p, "named case"))


# as trimmed by 2 (trim 3, one separator): no match, one, two, five; items that the trim empties
POOL = [b"", b"a", b"ab", b"abcXY", b"zabbcXY", b"abczz", b"abcabbc;;", b"zzabc abbbc\n\n", b"abc" * 5 + b"zz", b"abbcabcabcabbbcabc\x00\xff", b"zzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzabc..",
        b"\xffzz\x00", b"abbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbc12", b"abc"]


def pooled_batch(n, seed, lead):
    """n items drawn from POOL, each followed by one separator byte, `lead` bytes in front; built with numpy (n may pass a million).
    -> (text, offsets, index into POOL per item)."""
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


def pooled_csr(per, idx):
    """The CSR arrays of a batch drawn from a pool by `idx`, from the match list per pool item (numpy: the batch may pass a million)."""
    width = max(len(w) for w in per)
    pc = np.array([len(w) for w in per], dtype=np.int32)
    ps = np.zeros((len(per), width, 2), dtype=np.int32)
    for k, w in enumerate(per):
        ps[k, :len(w)] = np.array(w, dtype=np.int32).reshape(-1, 2)
    count = pc[idx]
    first = np.concatenate([[0], np.cumsum(count, dtype=np.int64)]).astype(np.int64)
    item_of_slot = np.repeat(np.arange(len(idx)), count)
    rank = np.arange(int(first[-1])) - first[item_of_slot]
    return count, first, ps[idx[item_of_slot], rank]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, MAX_BLOCKS_ITEMS + 65])
def test_batch_sizes(n):
    """Wave edges (63, 64, 65), workgroup edges (1023, 1024, 1025) and more items than one pass of the grid holds; the offsets do
    not begin at 0, the text tensor ends with the last item, and trim 3 is larger than some items (region = item + ';')."""
    p, trim, lead = "ab+c", 3, 16
    r = rr.RRegex(p)
    trimmed = [(it + b";")[:max(len(it) + 1 - trim, 0)] for it in POOL]
    per = [finditer_all(p, it) for it in trimmed]
    assert {len(w) for w in per} >= {0, 1, 2, 5} and any(len(it) + 1 < trim for it in POOL) and sum(not t for t in trimmed) >= 3
    short = [k for k, it in enumerate(trimmed) if len(it) <= 22]
    assert want_for(p, [trimmed[k] for k in short]) == [per[k] for k in short]       # (finditer and the oracle agree where both can tell)
    text, off, idx = pooled_batch(n, 40 + n % 7, lead)
    assert off[0] == lead != 0 and off[-1] == len(text)
    want = pooled_csr(per, idx)
    dev, doff = to_dev(text, off)
    assert dev.untyped_storage().nbytes() == int(off[-1])
    run_all_forms(r, dev, doff, trim, want, ("batch", n), caps=(None,) if n > 1025 else (None, 1, 0))
    assert n < 1023 or 0 < int((want[0] > 0).sum()) < n


def test_every_alignment_of_item_start_and_mark_word():
    """Items of 0 ... 100 bytes with a match at their first byte, one at their last and one in between, each item 32 times in a row
    at an odd pitch (an empty item in between where item + separator is even): (b - base) mod 32 takes all 32 residues and the byte
    address all 16, so every match starts at the first and at the last bit of a mark word and straddles one somewhere; then the
    whole buffer off 16-byte alignment."""
    p = "ab+c"
    shapes = []
    for length in (0, 1, 31, 32, 33, 63, 64, 65, 100):
        it = bytearray(b"z" * length)
        if length >= 31:
            it[0:3] = b"abc"
            it[length - 4:length] = b"abbc"
            it[13:19] = b"abbbbc"
        shapes.append(bytes(it))
    assert [len(s) for s in shapes] == [0, 1, 31, 32, 33, 63, 64, 65, 100]
    items = []
    for it in shapes:
        for _ in range(32):
            items += [it] if len(it) % 2 == 0 else [it, b""]       # pitch = item + separator (+ an empty item's separator): odd
    want_lists = [finditer_all(p, it) for it in items]
    assert {len(w) for w in want_lists} == {0, 3}
    want = csr(want_lists)
    r = rr.RRegex(p)
    for lead in (0, 3):
        text, offs = pack(items, 1, lead)
        base = int(offs[0])
        assert base == lead
        for shape in shapes:
            at = [int(o) for o, it in zip(offs[:-1], items) if it == shape]
            assert len({(o - base) % 32 for o in at}) == 32 and len({o % 16 for o in at}) == 16, (len(shape), lead)
        starts = {(int(o) - base + s) % 32 for o, w in zip(offs[:-1], want_lists) for s, _ in w}
        ends = {(int(o) - base + e) % 32 for o, w in zip(offs[:-1], want_lists) for _, e in w}
        straddling = sum((int(o) - base + s) % 32 + (e - s) > 32 for o, w in zip(offs[:-1], want_lists) for s, e in w)
        assert len(starts) == 32 and len(ends) == 32 and straddling > 50
        assert len({int(o) % 16 for o in offs[:-1]}) == 16
        dev, doff = to_dev(text, offs)
        assert dev.data_ptr() % 16 == 0
        run_all_forms(r, dev, doff, 1, want, ("alignment", lead), caps=(None,))
        run_all_forms(r, dev, doff, 1, want, ("alignment, indexed", lead), handle=rr.Items(dev, doff, trim=1), caps=(None,))
        sliced = torch.cat([torch.zeros(5, dtype=torch.uint8, device="cuda"), dev])[5:]
        assert sliced.data_ptr() % 16 == 5
        run_all_forms(r, sliced, doff, 1, want, ("alignment, sliced", lead), caps=(None,))


def test_long_items():
    """5 KB ... 100 KB per item, the expected lists from re.finditer: more than 10000 matches of [0-9]+ in one item of digits and
    blanks, one match of 30 KB, runs of 1000 'a' under a{1,300} (300, 300, 300, 100), items without a match - on the LDS tables
    and with both tables forced into HBM/L2."""
    rng = random.Random(41)
    fill = b"xy zb" * 20001                                         # (no 'a', no digit: no pattern matches inside it)
    sets = {}
    dense = bytes(rng.choice(b"0123456789   ") for _ in range(60000))
    sets["[0-9]+"] = [dense, fill[:5000], fill[:20000] + b"7" + fill[:17], b"12345" + fill[:65536] + b"678", fill[:100000], dense[:5001][::-1]]
    sets["ab+c"] = [fill[:40000] + b"a" + b"b" * 30000 + b"c" + fill[:16] + b"abc", fill[:65536], b"abc" + fill[:99990] + b"abbbbbc",
                    b"abc" * 2000, fill[:5001], fill[:4990] + b"abc" + fill[:15] + b"ab" + fill[:301] + b"abbc"]
    run = b"a" * 1000
    sets["a{1,300}"] = [fill[:7000] + run + fill[:33] + run, run + fill[:5000], fill[:100000], fill[:20000] + b"a" + fill[:1] + run, fill[:5000]]
    for p, items in sets.items():
        want_lists = [finditer_all(p, it) for it in items]
        counts = [len(w) for w in want_lists]
        assert all(5000 <= len(it) <= 135000 for it in items) and 0 < sum(c == 0 for c in counts) < len(items)
        if p == "[0-9]+":
            assert counts[0] > 10000
        elif p == "ab+c":
            assert max(e - s for w in want_lists for s, e in w) == 30002
        else:
            assert [e - s for s, e in want_lists[1]] == [300, 300, 300, 100] and [e - s for s, e in want_lists[0]] == [300, 300, 300, 100] * 2
        short = [it[-22:] for it in items]                          # the last 22 bytes: the brute force and finditer agree
        assert want_for(p, short) == [finditer_all(p, it) for it in short]
        want = csr(want_lists)
        for engine in (rr.ENGINE_AUTO, rr.ENGINE_DFA_GLOBAL):
            r = rr.RRegex(p, engine)
            for trim, lead in ((0, 0), (1, 7)):
                dev, doff = to_dev(*pack(items, trim, lead, seed=trim))
                run_all_forms(r, dev, doff, trim, want, (p, "long", engine, trim), caps=(None,))


def test_global_form():
    """RRX_ENGINE_DFA_GLOBAL forces both tables into HBM/L2; under AUTO, a pattern whose two tables pass 64 KiB goes there."""
    ref = reference_all()
    for p, items, want_lists in ref[:12] + ref[-len(NEWLINE_PATTERNS):]:
        dev, doff = to_dev(*pack(items, 1, lead=2))
        run_all_forms(rr.RRegex(p, rr.ENGINE_DFA_GLOBAL), dev, doff, 1, csr(want_lists), (p[:30], "global form"), caps=(None,))
    r = rr.RRegex(GLOBAL_AUTO)
    assert plain_table_bytes(r.program(rr.PROGRAM_SEARCH_STARTS)) + plain_table_bytes(r.program(rr.PROGRAM_SEARCH_ANCHORED)) > 65536
    items = global_auto_items(random.Random(42), 300)
    want_lists = want_for(GLOBAL_AUTO, items)
    # two matches in one item are beyond the brute force's 22 bytes: Python's greedy search names the longest here ([ab]* takes all)
    greedy = re.compile(rb"x[ab]{12}a[ab]*")
    assert all([(m.start(), m.end()) for m in greedy.finditer(it)] == w for it, w in zip(items, want_lists))
    more = [items[-5] + b"b" + items[-4], items[-3] + items[-5], b"x" + items[-5] + b"xx" + items[-4] + b"x"]
    items += more
    want_lists += [[(m.start(), m.end()) for m in greedy.finditer(it)] for it in more]
    assert 5 < sum(bool(w) for w in want_lists) < len(items) and sum(len(w) >= 2 for w in want_lists) >= 3
    for trim, lead in ((0, 0), (1, 9)):
        dev, doff = to_dev(*pack(items, trim, lead))
        run_all_forms(r, dev, doff, trim, csr(want_lists), ("AUTO, tables beyond the LDS budget", trim))


def poisoned(n):
    return torch.full((n,), POISON, dtype=torch.int32, device="cuda")


def mark_words_of(offs, trim, n):
    """The mark words that the items of a batch own: {((g - base) >> 5) + i for every byte g of item i}."""
    base, out = int(offs[0]), set()
    for i in range(n):
        b, e = SearchAllLongestReplay.span(offs, i, trim)
        if e > b:
            out |= set(range(((b - base) >> 5) + i, ((e - 1 - base) >> 5) + i + 1))
    return out


def test_edge_patterns_and_buffers():
    rng = random.Random(43)
    items = short_items(rng, "ab+c", 131) + [b"abcabbc;abc", b"abc" * 7, b""] + [b"z" * k + b"abbc" * 5 for k in range(3)]
    n = len(items)
    text, offs = pack(items, 1, lead=2)
    dev, doff = to_dev(text, offs)
    handle = rr.Items(dev, doff, trim=1)
    L, stream = rr._L, rr._stream_ptr(None)
    words = L.rrx_search_all_longest_marks_words(int(offs[-1] - offs[0]), n)
    owned = mark_words_of(offs, 1, n)
    assert max(owned) < words and len(owned) < words
    for p in ("ab+c", "a*", "[]"):
        r = rr.RRegex(p)
        want_lists = want_for(p, items)
        count, first, pairs = csr(want_lists)
        total = len(pairs)
        assert p == "[]" or total > n // 4
        # a gap of one slot in front of the second half's matches: _fill must leave it alone
        gap_at = n // 2
        gapped = first[:n] + (np.arange(n) >= gap_at)
        d_first = torch.from_numpy(gapped.copy()).cuda()
        gap_slot = int(first[gap_at])
        for indexed in (False, True):
            # _count writes exactly nitems words and the items' mark words, _fill exactly the slots of the prefix
            cnt, marks, st, en = poisoned(n + 1), poisoned(words + 1), poisoned(total + 2), poisoned(total + 2)
            if indexed:
                rr._check(L.rrx_search_all_longest_items_count(r._h, handle._h, marks.data_ptr(), words, cnt.data_ptr(), stream))
                rr._check(L.rrx_search_all_longest_items_fill(r._h, handle._h, marks.data_ptr(), words, d_first.data_ptr(), st.data_ptr(), en.data_ptr(), stream))
            else:
                rr._check(L.rrx_search_all_longest_extents_count(r._h, 0, dev.data_ptr(), doff.data_ptr(), n, 1, marks.data_ptr(), words, cnt.data_ptr(), stream))
                rr._check(L.rrx_search_all_longest_extents_fill(r._h, 0, dev.data_ptr(), doff.data_ptr(), n, 1, marks.data_ptr(), words, d_first.data_ptr(),
                                                                st.data_ptr(), en.data_ptr(), stream))
            torch.cuda.synchronize()
            assert int(cnt[n]) == POISON and int(marks[words]) == POISON and int(st[total + 1]) == POISON and int(en[total + 1]) == POISON, (p, indexed)
            assert (cnt[:n] != POISON).all(), (p, indexed, "a count word was not written")
            assert np.array_equal(cnt[:n].cpu().numpy(), count), (p, indexed, "count")
            m = marks[:words].cpu().numpy()
            touched = set(np.nonzero(m != POISON)[0].tolist())
            if p == "ab+c":                          # every word of the items' ranges, all-zero words included, and no other (no mark
                assert touched == owned, (p, indexed, sorted(touched ^ owned)[:5])      # word equals the poison: two matches of ab+c never start side by side)
            else:                                   # a nullable pattern and the empty language never touch the marks
                assert not touched, (p, indexed)
            gs, ge = st.cpu().numpy(), en.cpu().numpy()
            assert gs[gap_slot] == POISON and ge[gap_slot] == POISON, (p, indexed, "the gap was written")
            keep = np.arange(total + 1) != gap_slot
            assert np.array_equal(np.stack([gs[:total + 1][keep], ge[:total + 1][keep]], axis=1), pairs), (p, indexed, "fill")
            # the one-call form with cap < total: d_first complete, slots >= cap untouched, the retry exact
            for cap in (total // 2, 0, total):
                fst, st, en, tot = torch.full((n + 2,), POISON, dtype=torch.int64, device="cuda"), poisoned(total + 1), poisoned(total + 1), C.c_size_t(99)
                if indexed:
                    rr._check(L.rrx_search_all_longest_items(r._h, handle._h, fst.data_ptr(), st.data_ptr(), en.data_ptr(), cap, C.byref(tot), stream))
                else:
                    rr._check(L.rrx_search_all_longest_extents(r._h, 0, dev.data_ptr(), doff.data_ptr(), n, 1, fst.data_ptr(), st.data_ptr(), en.data_ptr(), cap,
                                                               C.byref(tot), stream))
                torch.cuda.synchronize()
                assert tot.value == total and int(fst[n + 1]) == POISON and np.array_equal(fst[:n + 1].cpu().numpy(), first), (p, indexed, cap)
                assert (st[cap:] == POISON).all() and (en[cap:] == POISON).all(), (p, indexed, cap, "a slot >= cap was written")
                assert np.array_equal(torch.stack([st[:cap], en[:cap]], dim=1).cpu().numpy(), pairs[:cap]), (p, indexed, cap)
    r, tot = rr.RRegex("ab+c"), C.c_size_t(0)
    # cap == 0 needs no match arrays
    fst = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    rr._check(L.rrx_search_all_longest_extents(r._h, 0, dev.data_ptr(), doff.data_ptr(), n, 1, fst.data_ptr(), None, None, 0, C.byref(tot), stream))
    assert tot.value == int(fst[-1]) == len(csr(want_for("ab+c", items))[2])
    assert L.rrx_search_all_longest_extents(r._h, 0, dev.data_ptr(), doff.data_ptr(), n, 1, fst.data_ptr(), None, None, 5, C.byref(tot), stream) == 2      # RRX_ERR_ARG
    cnt, marks = poisoned(n), poisoned(words)
    assert L.rrx_search_all_longest_extents_count(r._h, 0, dev.data_ptr(), doff.data_ptr(), n, 1, marks.data_ptr(), n, cnt.data_ptr(), stream) == 2        # marks_words < n + 1
    assert L.rrx_search_all_longest_items_count(r._h, handle._h, marks.data_ptr(), n, cnt.data_ptr(), stream) == 2
    assert L.rrx_search_all_longest_items_fill(r._h, handle._h, marks.data_ptr(), n, fst.data_ptr(), cnt.data_ptr(), cnt.data_ptr(), stream) == 2
    torch.cuda.synchronize()
    assert (cnt == POISON).all() and (marks == POISON).all()
    # a regex whose tables do not determinise: RRX_ERR_UNSUPPORTED, nothing written
    bad = rr.RRegex(EXPLODING)
    st = poisoned(8)
    assert L.rrx_search_all_longest_extents_count(bad._h, 0, dev.data_ptr(), doff.data_ptr(), n, 1, marks.data_ptr(), words, cnt.data_ptr(), stream) == 4
    assert b"determinise" in L.rrx_last_error()
    assert L.rrx_search_all_longest_items_count(bad._h, handle._h, marks.data_ptr(), words, cnt.data_ptr(), stream) == 4
    assert L.rrx_search_all_longest_extents_fill(bad._h, 0, dev.data_ptr(), doff.data_ptr(), n, 1, marks.data_ptr(), words, d_first.data_ptr(), st.data_ptr(),
                                                 st.data_ptr(), stream) == 4
    assert L.rrx_search_all_longest_items_fill(bad._h, handle._h, marks.data_ptr(), words, d_first.data_ptr(), st.data_ptr(), st.data_ptr(), stream) == 4
    fst = torch.full((n + 1,), POISON, dtype=torch.int64, device="cuda")
    assert L.rrx_search_all_longest_extents(bad._h, 0, dev.data_ptr(), doff.data_ptr(), n, 1, fst.data_ptr(), st.data_ptr(), st.data_ptr(), 8, C.byref(tot), stream) == 4
    assert L.rrx_search_all_longest_items(bad._h, handle._h, fst.data_ptr(), st.data_ptr(), st.data_ptr(), 8, C.byref(tot), stream) == 4
    torch.cuda.synchronize()
    assert (cnt == POISON).all() and (marks == POISON).all() and (st == POISON).all() and (fst == POISON).all()
    # all-empty items: nothing but offsets; an empty batch: first[0] = 0; a trim larger than every item
    nothing = torch.empty(0, dtype=torch.uint8, device="cuda")
    zero = torch.zeros(1, dtype=torch.int64, device="cuda")
    off0 = torch.zeros(71, dtype=torch.int64, device="cuda")
    run_all_forms(r, nothing, off0, 0, csr([[]] * 70), "all-empty items")
    run_all_forms(rr.RRegex("a*"), nothing, off0, 0, csr([[(0, 0)]] * 70), "all-empty items, nullable")
    run_all_forms(r, dev, doff, 100, csr([[]] * n), "a trim larger than every item")
    run_all_forms(rr.RRegex("a*"), dev, doff, 100, csr([[(0, 0)]] * n), "a trim larger than every item, nullable")
    for rx in (r, rr.RRegex("a*"), rr.RRegex("[]")):
        run_all_forms(rx, nothing, zero, 0, csr([]), "empty batch")
        run_all_forms(rx, nothing, zero, 0, csr([]), "empty batch", handle=rr.Items(nothing, zero))
    for call in (lambda: bad.search_all_longest_extents(nothing, zero), lambda: bad.search_all_longest_items(rr.Items(nothing, zero)),
                 lambda: bad.search_all_longest_extents_fused(nothing, zero), lambda: bad.search_all_longest_items_fused(rr.Items(nothing, zero)),
                 lambda: bad.search_all_longest_extents(dev, doff, trim=1), lambda: bad.search_all_longest_items_fused(handle)):
        with pytest.raises(rr.RRegexError, match="determinise"):
            call()


@pytest.mark.parametrize("kind", ["url", "email", "kwlog"])
def test_large_text_against_the_first_match_the_lazy_count_and_the_replay(kind):
    """16 MiB of '\\n' text viewed as items - offsets = the line starts, trim 1.  The first match of every item is
    rrx_search_longest_extents' answer, count > 0 exactly where that entry finds one; the matches of an item ascend without overlap
    and none is empty; no item has more matches than rrx_search_all_extents_count finds (earliest-end-first is a maximum set of
    disjoint matches); the indexed batch gives the same; 300 sampled items against the CPU replay of kinds 19 / 20 and the marks."""
    import synth
    pattern = {"url": U2, "email": EMAIL, "kwlog": K1000_CONTAINS}[kind]
    host = synth.corpus(kind, 6, 16 << 20)
    host = host[:int(np.nonzero(host == 10)[0][-1]) + 1]                 # (whole lines: every item has its separator)
    r = rr.RRegex(pattern)
    assert not r.accepts_empty
    dev = torch.from_numpy(host).cuda()
    off = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.nonzero(dev == 10).flatten() + 1]).contiguous()
    n = off.numel() - 1
    ls, le = r.search_longest_extents(dev, off, trim=1)
    gc, gf, gs, ge = r.search_all_longest_extents(dev, off, trim=1)
    found = le >= 0
    total = gs.numel()
    assert 0 < int(found.sum()) and (kind == "kwlog" or int(found.sum()) < n)
    assert torch.equal(gc > 0, found), (kind, "found-ness")
    assert total == int(gc.sum()) and torch.equal(gf, torch.cumsum(gc, 0, dtype=torch.int64) - gc)
    assert torch.equal(gs[gf[found]], ls[found]) and torch.equal(ge[gf[found]], le[found]), (kind, "the first match")
    assert bool((gs < ge).all()) and bool((gs >= 0).all())
    is_first = torch.zeros(total, dtype=torch.bool, device="cuda")
    is_first[gf[found]] = True
    assert bool(((gs[1:] >= ge[:-1]) | is_first[1:]).all()), (kind, "ascending, no overlap")
    lens = (off[1:] - off[:-1] - 1).clamp(min=0)
    last = (gf + gc - 1)[found]
    assert bool((ge[last] <= lens[found]).all()), (kind, "inside the item")
    lazy = r.search_all_extents(dev, off, trim=1)[0]
    assert bool((gc <= lazy).all()), (kind, "more matches than earliest-end-first")
    ic, if_, is_, ie = r.search_all_longest_items(rr.Items(dev, off, trim=1))
    assert torch.equal(ic, gc) and torch.equal(if_, gf) and torch.equal(is_, gs) and torch.equal(ie, ge), (kind, "indexed")
    ff, fs, fe = r.search_all_longest_extents_fused(dev, off, trim=1, cap=total)
    assert torch.equal(ff[:-1], gf) and int(ff[-1]) == total and torch.equal(fs, gs) and torch.equal(fe, ge), (kind, "one call")
    sample = np.sort(np.random.default_rng(9).choice(n, size=300, replace=False))
    offs = off.cpu().numpy()
    items = [host[offs[k]:offs[k + 1] - 1].tobytes() for k in sample]
    want = SearchAllLongestReplay(r).run(items, trim=1, lead=3)
    c, f, s, e = gc.cpu().numpy(), gf.cpu().numpy(), gs.cpu().numpy(), ge.cpu().numpy()
    got = [list(zip(s[f[k]:f[k] + c[k]].tolist(), e[f[k]:f[k] + c[k]].tolist())) for k in sample]
    assert got == want, (kind, "replay", next(k for k in range(300) if got[k] != want[k]))
    assert sum(len(w) for w in want) > 0


def test_a_side_stream_and_two_captured_graphs():
    p, items, want_lists = next(x for x in reference_all() if x[0] == "[ab]{1,2}b*a*")      # (of the shared patterns one with many matches: 156, two or more in 39 items)
    items = list(items)
    want = csr(want_lists)
    n, total = len(items), len(want[2])
    assert not rr.RRegex(p).accepts_empty and total > n // 2 and sum(len(w) >= 2 for w in want_lists) > 20
    r = rr.RRegex(p)
    text, offs = pack(items, 1, lead=1)
    dev, doff = to_dev(text, offs)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    got = r.search_all_longest_extents(dev, doff, trim=1, stream=side)       # (eager: the tables are uploaded here)
    fused = r.search_all_longest_extents_fused(dev, doff, trim=1, stream=side)
    side.synchronize()
    assert_csr(got, want, "side stream")
    assert_csr((None,) + fused, want, "side stream, one call")
    # _count and _fill captured into a graph each (the tables are up: nothing is allocated or uploaded inside a capture), the prefix
    # computed on the device between the two replays; replayed on refilled inputs: the same items in another order have the same total
    words = rr._L.rrx_search_all_longest_marks_words(len(text), n)
    cnt, marks, st, en = poisoned(n), poisoned(words), poisoned(total), poisoned(total)
    first = torch.zeros(n, dtype=torch.int64, device="cuda")
    g_count, g_fill = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    s = rr._stream_ptr(side)
    with torch.cuda.stream(side):
        with torch.cuda.graph(g_count, stream=side):
            rr._check(rr._L.rrx_search_all_longest_extents_count(r._h, 0, dev.data_ptr(), doff.data_ptr(), n, 1, marks.data_ptr(), words, cnt.data_ptr(), s))
        with torch.cuda.graph(g_fill, stream=side):
            rr._check(rr._L.rrx_search_all_longest_extents_fill(r._h, 0, dev.data_ptr(), doff.data_ptr(), n, 1, marks.data_ptr(), words, first.data_ptr(),
                                                                st.data_ptr(), en.data_ptr(), s))
    torch.cuda.current_stream().wait_stream(side)
    for round_, order in enumerate((list(range(n)), list(reversed(range(n))))):
        shuffled = [items[k] for k in order]
        text2, offs2 = pack(shuffled, 1, lead=1)
        assert len(text2) == len(text)
        dev.copy_(torch.from_numpy(text2))
        doff.copy_(torch.from_numpy(offs2))
        for t in (cnt, marks, st, en):
            t.fill_(POISON)
        g_count.replay()
        first.copy_(torch.cumsum(cnt, dim=0, dtype=torch.int64) - cnt)      # the prefix on the device, outside the captures
        g_fill.replay()
        torch.cuda.synchronize()
        want2 = csr([want_lists[k] for k in order])
        assert_csr((cnt, first, st, en), want2, ("replay", round_))
        assert_csr(r.search_all_longest_extents(dev, doff, trim=1), want2, ("direct call", round_))
