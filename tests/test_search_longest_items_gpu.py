"""rrx_search_longest_extents / rrx_search_longest_items on the device: per item the LEFTMOST-LONGEST accepted substring - the
smallest start, then the largest end.  Against the oracle's brute force on short items (the CPU test's patterns, items and
expected values), Python's re on patterns for which its greedy search names the same substring (test_search_longest_items_lowering
checks that), and on large text the CPU replay of the two tables plus the invariants that tie the answer to rrx_search_extents'."""
import random
import re

import numpy as np
import pytest

import roaringregex_amd as rr
from contains_cases import EXPLODING
from patterns import EMAIL, K1000_CONTAINS, U2
from test_contains_items_lowering import NEWLINE_PATTERNS, short_items
from table_edge_cases import plain_table_bytes
from test_search_longest_items_lowering import GLOBAL_AUTO, GREEDY_RE, START_CASES, SearchLongestReplay, global_auto_items, reference_set, want_for

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
MAX_BLOCKS_ITEMS = 1024 * 1024                      # kernels_search_longest_items.hip: 1024 workgroups of 1024 lanes, then the grid strides


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"


def pack(items, trim, lead=0, seed=0):
    """items -> (text, offsets): every item followed by `trim` separator bytes of any value, `lead` bytes in front of the first; the
    text ends with the last item's separators."""
    rng = random.Random(seed)
    seps = b"ab\n;\x00\xffc"
    parts, offs, at = [b"q" * lead], [lead], lead
    for it in items:
        parts.append(it + bytes(rng.choice(seps) for _ in range(trim)))
        at += len(it) + trim
        offs.append(at)
    return np.frombuffer(b"".join(parts), dtype=np.uint8).copy(), np.array(offs, dtype=np.int64)


def to_dev(text, offs):
    d = torch.from_numpy(text).cuda() if len(text) else torch.empty(0, dtype=torch.uint8, device="cuda")
    return d, torch.from_numpy(offs).cuda()


def as_pairs(start, end):
    return torch.stack([start, end], dim=1).cpu().numpy()


def assert_same(got, want, what, items=None):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (what, "first bad item", int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist(), None if items is None else items[bad[0]][:60])


def run_extents(r, items, want, trim, what, lead=0):
    dev, doff = to_dev(*pack(items, trim, lead, seed=len(items)))
    assert_same(as_pairs(*r.search_longest_extents(dev, doff, trim=trim)), want, what, items)


def greedy_want(p, items):
    c = re.compile(GREEDY_RE[p])
    ms = [c.search(it) for it in items]
    return np.array([(m.start(), m.end()) if m else (-1, -1) for m in ms], dtype=np.int32).reshape(len(items), 2)


def test_short_items_against_the_brute_force():
    """One call with trim 0, one call with a separator byte per item (trim 1), and the indexed batch at both trims; then the
    hand-made items whose start differs from the smallest-end answer."""
    for p, items, want, _ in reference_set():
        r = rr.RRegex(p)
        run_extents(r, items, want, 0, (p[:30], "trim 0"))
        run_extents(r, items, want, 1, (p[:30], "trim 1"))
        dev, doff = to_dev(*pack(items, 1, seed=7))
        assert_same(as_pairs(*r.search_longest_items(rr.Items(dev, doff, trim=1))), want, (p[:30], "indexed trim 1"), items)
        dev0, doff0 = to_dev(*pack(items, 0))
        assert_same(as_pairs(*r.search_longest_items(rr.Items(dev0, doff0))), want, (p[:30], "indexed trim 0"), items)
    for p, item in START_CASES + [("[0-9]+", b"abc 12345 x"), ("ab|b+", b"abbb")]:
        run_extents(rr.RRegex(p), [item] * 3, want_for(p, [item] * 3), 1, (p, "named case"), lead=3)


POOL = [b"", b"a", b"c", b"abc", b"zabbc", b"ab", b"abcabc", b"\nabc", b"ab\nc", b"zzzzzzzzzzzzzzzzzabbbc", b"\xffabc\x00", b"bc", b"aabbcc",
        b"abcc", b"zzzzzzzzzzzzzzzabc", b"zzzzzzzzzzzzzzzzabc", b"zzzzzzzzzzzzzabc", b"abbbbbbbbbbbbbbbbbbbbc", b"abbbbbbbbbbbbbbbbbbbbb"]


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


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, MAX_BLOCKS_ITEMS + 65])
def test_batch_sizes(n):
    """Wave edges (63, 64, 65), workgroup edges (1023, 1024, 1025) and more items than one pass of the grid holds; the offsets do
    not begin at 0, the text tensor ends with the last item, and trim 3 is larger than some items (region = item + ';').  The
    expected value of every pool entry is the oracle's brute force on the entry as trimmed."""
    p = "ab+c"
    r = rr.RRegex(p)
    for trim, lead in ((1, 5), (3, 16)) if n <= 1025 else ((3, 16),):
        text, off, idx = pooled_batch(n, 40 + n % 7, lead)
        assert off[0] == lead != 0 and off[-1] == len(text)
        trimmed = [(it + b";")[:max(len(it) + 1 - trim, 0)] for it in POOL]
        assert trim == 1 or any(len(it) + 1 < trim for it in POOL)
        want = want_for(p, trimmed)[idx]
        dev, doff = to_dev(text, off)
        assert dev.untyped_storage().nbytes() == int(off[-1])
        got = as_pairs(*r.search_longest_extents(dev, doff, trim=trim))
        assert_same(got, want, ("batch", n, trim))
        assert 0 < int((want[:, 1] >= 0).sum()) < n or n == 1


def test_every_alignment_of_item_start_match_start_and_match_end():
    """Items of 0 ... 40 bytes with one match at every offset, each placed at all 16 alignments of its first byte (an item of L bytes
    with its separator, 16 copies in a row, L + 1 odd or padded to odd: consecutive copies walk through the 16 residues): the tail /
    wide / head split of the backward walk and the head / wide / tail split of the forward walk both see every residue of the item
    start, the match start and the match end."""
    p = "ab+c"
    items = []
    for length in (0, 1, 15, 16, 17, 31, 32, 33, 40):
        for needle in (b"abc", b"abbbbbbbbbbbbbbbbbbbc"):          # (the long one: both walks cross a 16-byte boundary inside the match)
            for at in range(max(length - len(needle) + 1, 0)):
                it = b"z" * at + needle + b"z" * (length - at - len(needle))
                assert len(it) == length
                items += [it, it + b"z"] * 8 if length % 2 else [it] * 16      # regions of odd length: 16 copies, 16 residues
        if length < 3:
            items += [b"z" * length] * 16
    want = greedy_want(p, items)
    lens = {len(it) for it in items}
    assert lens >= {0, 1, 15, 16, 17, 31, 32, 33, 40}
    assert {int(e) for e in want[:, 1]} >= {3, 15, 16, 17, 31, 32, 33, 40} and {int(s) for s in want[:, 0]} >= {0, 1, 15, 16, 17, 19}
    r = rr.RRegex(p)
    for lead in (0, 3):
        text, offs = pack(items, 1, lead)
        found = want[:, 1] >= 0
        residues = {(int(o), int(o + s) % 16, int(o + e) % 16) for o, (s, e) in zip((offs[:-1] % 16)[found], want[found])}
        assert len({x[0] for x in residues}) == 16 and len({x[1] for x in residues}) == 16 and len({x[2] for x in residues}) == 16
        dev, doff = to_dev(text, offs)
        assert dev.data_ptr() % 16 == 0
        assert_same(as_pairs(*r.search_longest_extents(dev, doff, trim=1)), want, ("alignment", lead), items)
        # ... and with the byte buffer itself off 16-byte alignment (a slice of a tensor)
        sliced = torch.cat([torch.zeros(5, dtype=torch.uint8, device="cuda"), dev])[5:]
        assert sliced.data_ptr() % 16 == 5
        assert_same(as_pairs(*r.search_longest_extents(sliced, doff, trim=1)), want, ("alignment, sliced", lead), items)


def test_long_items():
    """5 KB ... 100 KB per item: a planted match near the end, at the very start, at the very end; a match of 30 KB; a match as long
    as the pattern allows inside a longer run; items without a match."""
    rng = random.Random(31)
    fill = b"xy zb" * 20001                                         # (no 'a': neither pattern matches inside it)
    for p, needles in (("ab+c", [b"abc", b"abbbbbc", b"a" + b"b" * 30000 + b"c"]), ("a{1,300}", [b"a", b"a" * 1000])):
        items = []
        for k in range(40):
            n = rng.choice([5000, 5001, 20000, 65536, 100000])
            needle = needles[k % len(needles)]
            tail = 0 if k % 7 == 3 else rng.choice([1, 15, 16, 17, 300])
            head = 0 if k % 7 == 5 else max(n - len(needle) - tail, 0)
            it = fill[:head] + needle + fill[:tail if head else max(n - len(needle), 0)]
            items.append(it if k % 9 else fill[:n])                 # one item in nine has no match
        want = greedy_want(p, items)
        found = want[:, 1] >= 0
        assert 0 < int((~found).sum()) < len(items) and int(want[:, 1].max()) > 99000
        assert (want[found, 0] == 0).any() and any(int(e) == len(it) for it, e in zip(items, want[:, 1]))      # at the very start, at the very end
        if p == "a{1,300}":                                         # the longest: 300 bytes into a run of 1000, the whole run of one
            assert {int(x) for x in want[found, 1] - want[found, 0]} == {1, 300}
        else:
            assert int((want[:, 1] - want[:, 0]).max()) == 30002
        short = [it[-22:] for it in items]                          # the last 22 bytes: the brute force and the greedy search agree
        assert (want_for(p, short) == greedy_want(p, short)).all()
        r = rr.RRegex(p)
        run_extents(r, items, want, 0, (p, "long, trim 0"))
        run_extents(r, items, want, 1, (p, "long, trim 1"), lead=7)
        run_extents(rr.RRegex(p, rr.ENGINE_DFA_GLOBAL), items, want, 1, (p, "long, global form"))


def test_global_form():
    """RRX_ENGINE_DFA_GLOBAL forces both tables into HBM/L2; under AUTO, a pattern whose two tables pass 64 KiB goes there."""
    ref = reference_set()
    for p, items, want, _ in ref[:12] + ref[-len(NEWLINE_PATTERNS):]:
        run_extents(rr.RRegex(p, rr.ENGINE_DFA_GLOBAL), items, want, 1, (p[:30], "global form"))
    r = rr.RRegex(GLOBAL_AUTO)
    assert plain_table_bytes(r.program(rr.PROGRAM_SEARCH_STARTS)) + plain_table_bytes(r.program(rr.PROGRAM_SEARCH_ANCHORED)) > 65536
    items = global_auto_items(random.Random(32), 300)
    want = want_for(GLOBAL_AUTO, items)
    assert 5 < int((want[:, 1] >= 0).sum()) < len(items)
    run_extents(r, items, want, 0, "AUTO, tables beyond the LDS budget")
    run_extents(r, items, want, 1, "AUTO, tables beyond the LDS budget, trim 1", lead=9)


def test_edge_patterns_and_output_buffers():
    rng = random.Random(33)
    items = short_items(rng, "ab+c", 131)
    text, offs = pack(items, 1, lead=2)
    dev, doff = to_dev(text, offs)
    n = len(items)
    handle = rr.Items(dev, doff, trim=1)

    def poisoned(r, indexed, expect_rc=0):
        """Both entries through the C ABI on buffers full of 0x5A5A5A5A, one word longer than needed."""
        st = torch.full((n + 1,), POISON, dtype=torch.int32, device="cuda")
        en = torch.full((n + 1,), POISON, dtype=torch.int32, device="cuda")
        stream = rr._stream_ptr(None)
        if indexed:
            rc = rr._L.rrx_search_longest_items(r._h, handle._h, st.data_ptr(), en.data_ptr(), stream)
        else:
            rc = rr._L.rrx_search_longest_extents(r._h, 0, dev.data_ptr(), doff.data_ptr(), n, 1, st.data_ptr(), en.data_ptr(), stream)
        assert rc == expect_rc, (rc, rr._L.rrx_last_error())
        torch.cuda.synchronize()
        assert int(st[n]) == POISON and int(en[n]) == POISON, "a word behind the results was written"
        got = as_pairs(st[:n], en[:n])
        if expect_rc:
            assert (got == POISON).all(), "a failed call wrote a result word"
        else:
            assert (got != POISON).all(), "a result word was not written"
        return got

    for indexed in (False, True):
        assert_same(poisoned(rr.RRegex("ab+c"), indexed), want_for("ab+c", items), ("poisoned", indexed), items)
        want = want_for("a*", items)                                                 # nullable: start 0, the longest accepted prefix
        assert (want[:, 0] == 0).all() and (want[:, 1] > 0).any() and (want[:, 1] == 0).any()
        assert_same(poisoned(rr.RRegex("a*"), indexed), want, ("nullable", indexed), items)
        assert (poisoned(rr.RRegex("[]"), indexed) == -1).all()                      # the empty language
        poisoned(rr.RRegex(EXPLODING), indexed, expect_rc=4)                         # RRX_ERR_UNSUPPORTED: nothing written
        assert b"determinise" in rr._L.rrx_last_error()
    bad = rr.RRegex(EXPLODING)
    nothing = torch.empty(0, dtype=torch.uint8, device="cuda")
    zero = torch.zeros(1, dtype=torch.int64, device="cuda")
    with pytest.raises(rr.RRegexError, match="determinise"):
        bad.search_longest_extents(nothing, zero)                                    # ... with zero items as well
    with pytest.raises(rr.RRegexError, match="determinise"):
        bad.search_longest_items(rr.Items(nothing, zero))
    # an empty batch writes nothing
    r = rr.RRegex("ab+c")
    s, e = r.search_longest_extents(nothing, zero)
    assert s.numel() == 0 and e.numel() == 0
    s, e = r.search_longest_items(rr.Items(nothing, zero))
    assert s.numel() == 0 and e.numel() == 0
    # all-empty items: nothing but offsets
    off0 = torch.zeros(70, dtype=torch.int64, device="cuda")
    assert (as_pairs(*r.search_longest_extents(nothing, off0)) == -1).all()
    assert (as_pairs(*rr.RRegex("a*").search_longest_extents(nothing, off0)) == 0).all()
    # a trim larger than every item: all items empty
    assert (as_pairs(*r.search_longest_extents(dev, doff, trim=100)) == -1).all()
    assert (as_pairs(*rr.RRegex("a*").search_longest_extents(dev, doff, trim=100)) == 0).all()
    assert rr._L.rrx_search_longest_extents(r._h, 0, dev.data_ptr(), doff.data_ptr(), 5, 0, None, None, None) == 2      # RRX_ERR_ARG


@pytest.mark.parametrize("kind", ["url", "email", "kwlog"])
def test_large_text_against_search_extents_and_the_replay(kind):
    """16 MiB of '\\n' text viewed as items - offsets = the line starts, trim 1.  For every item: found exactly where
    rrx_search_extents finds, start <= its start, end >= its end.  A fixed sample of 300 items against the CPU replay of kinds 19/20."""
    import synth
    pattern = {"url": U2, "email": EMAIL, "kwlog": K1000_CONTAINS}[kind]
    host = synth.corpus(kind, 6, 16 << 20)
    host = host[:int(np.nonzero(host == 10)[0][-1]) + 1]                 # (whole lines: every item has its separator)
    r = rr.RRegex(pattern)
    dev = torch.from_numpy(host).cuda()
    off = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.nonzero(dev == 10).flatten() + 1]).contiguous()
    n = off.numel() - 1
    ss, se = r.search_extents(dev, off, trim=1)
    gs, ge = r.search_longest_extents(dev, off, trim=1)
    found = se >= 0
    assert 0 < int(found.sum()) and (kind == "kwlog" or int(found.sum()) < n)
    assert torch.equal(ge >= 0, found) and torch.equal(gs >= 0, found), (kind, "found-ness")
    assert bool((gs[found] <= ss[found]).all()) and bool((ge[found] >= se[found]).all()), kind
    assert bool((gs[found] < ge[found]).all())
    is_, ie = r.search_longest_items(rr.Items(dev, off, trim=1))
    assert torch.equal(is_, gs) and torch.equal(ie, ge), (kind, "indexed")
    sample = np.random.default_rng(9).choice(n, size=300, replace=False)
    offs = off.cpu().numpy()
    items = [host[offs[k]:offs[k + 1] - 1].tobytes() for k in sample]
    want = SearchLongestReplay(r).search_items(items)
    assert_same(as_pairs(gs, ge)[sample], want, (kind, "replay"), items)
    assert int((want[:, 1] >= 0).sum()) > 0


def test_a_side_stream_and_a_captured_graph():
    p, items, want, _ = next(x for x in reference_set() if x[0] == EMAIL)
    items = list(items)
    r = rr.RRegex(p)
    text, offs = pack(items, 1, lead=1)
    dev, doff = to_dev(text, offs)
    n = len(items)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    s, e = r.search_longest_extents(dev, doff, trim=1, stream=side)      # (eager: the tables are uploaded here)
    side.synchronize()
    assert_same(as_pairs(s, e), want, "side stream", items)
    # one call captured (the tables are up: nothing is allocated or uploaded inside the capture), replayed twice on refilled inputs
    # and changed result buffers
    st = torch.full((n,), POISON, dtype=torch.int32, device="cuda")
    en = torch.full((n,), POISON, dtype=torch.int32, device="cuda")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            rr._check(rr._L.rrx_search_longest_extents(r._h, 0, dev.data_ptr(), doff.data_ptr(), n, 1, st.data_ptr(), en.data_ptr(), rr._stream_ptr(side)))
    torch.cuda.current_stream().wait_stream(side)
    for round_, order in enumerate((list(range(n)), list(reversed(range(n))))):
        shuffled = [items[k] for k in order]
        text2, offs2 = pack(shuffled, 1, lead=1)
        assert len(text2) == len(text)
        dev.copy_(torch.from_numpy(text2))
        doff.copy_(torch.from_numpy(offs2))
        st.fill_(POISON)
        en.fill_(POISON)
        g.replay()
        torch.cuda.synchronize()
        assert_same(as_pairs(st, en), want[order], ("replay", round_), shuffled)
        assert_same(as_pairs(*r.search_longest_extents(dev, doff, trim=1)), want[order], ("direct call", round_), shuffled)
