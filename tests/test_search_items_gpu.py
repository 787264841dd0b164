"""rrx_search_extents / rrx_search_items on the device: per item the accepted substring with the smallest end, then the smallest
start.  Against the oracle's brute force on short items (the CPU test's patterns, items and replay reference), Python's re on
patterns for which its lazy search names the same substring (test_search_items_lowering checks that), and rrx_search_corpus
element for element on '\\n' text viewed as items."""
import random
import re

import numpy as np
import pytest

import roaringregex_amd as rr
from contains_cases import EXPLODING, short_line_patterns
from patterns import EMAIL, K1000_CONTAINS, U2
from test_contains_items_lowering import NEWLINE_PATTERNS, short_items
from test_search_items_lowering import GLOBAL_AUTO, LAZY_RE, NITEMS, plain_table_bytes, want_for

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
MAX_BLOCKS_ITEMS = 1024 * 1024                      # kernels_search_items.hip: 1024 workgroups of 1024 lanes, then the grid strides


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"


@pytest.fixture(scope="module")
def reference():
    """[(pattern, items, want)]: the CPU test's patterns, items (same seed) and brute force - computed once, never changed."""
    rng = random.Random(1901)
    out = []
    for p in short_line_patterns() + NEWLINE_PATTERNS:
        items = short_items(rng, p, NITEMS)
        want = want_for(p, items)
        want.setflags(write=False)
        out.append((p, items, want))
    return out


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
    assert_same(as_pairs(*r.search_extents(dev, doff, trim=trim)), want, what, items)


def lazy_want(p, items):
    c = re.compile(LAZY_RE[p])
    ms = [c.search(it) for it in items]
    return np.array([(m.start(), m.end()) if m else (-1, -1) for m in ms], dtype=np.int32).reshape(len(items), 2)


def re_brute_force(rx, item):
    """Smallest end, then smallest start, with Python's fullmatch (patterns whose syntax the dialects share)."""
    c = re.compile(rx)
    for e in range(1, len(item) + 1):
        for s in range(e):
            if c.fullmatch(item, s, e):
                return s, e
    return -1, -1


def test_short_items_against_the_brute_force(reference):
    """One call with trim 0, one call with a separator byte per item (trim 1), and the indexed batch."""
    for p, items, want in reference:
        r = rr.RRegex(p)
        run_extents(r, items, want, 0, (p[:30], "trim 0"))
        run_extents(r, items, want, 1, (p[:30], "trim 1"))
        dev, doff = to_dev(*pack(items, 1, seed=7))
        handle = rr.Items(dev, doff, trim=1)
        assert_same(as_pairs(*r.search_items(handle)), want, (p[:30], "indexed trim 1"), items)
        dev0, doff0 = to_dev(*pack(items, 0))
        assert_same(as_pairs(*r.search_items(rr.Items(dev0, doff0))), want, (p[:30], "indexed trim 0"), items)


POOL = [b"", b"a", b"c", b"abc", b"zabbc", b"ab", b"abcabc", b"\nabc", b"ab\nc", b"zzzzzzzzzzzzzzzzzabbbc", b"\xffabc\x00", b"bc", b"aabbcc",
        b"abcc", b"zzzzzzzzzzzzzzzabc", b"zzzzzzzzzzzzzzzzabc", b"zzzzzzzzzzzzzabc", b"abbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbc", b"ab" * 20]


def pooled_batch(n, seed, trim, lead):
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


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130, 4097, MAX_BLOCKS_ITEMS + 65])
def test_batch_sizes(n):
    """Wave edges (63, 64, 65, 130), more than one workgroup (4097) and more items than one pass of the grid holds; the offsets do
    not begin at 0, the text tensor ends with the last item, and trim 3 is larger than some items (region = item + ';')."""
    p = "ab+c"
    r = rr.RRegex(p)
    for trim, lead in ((1, 5), (3, 16)) if n <= 4097 else ((3, 16),):
        text, off, idx = pooled_batch(n, 40 + n % 7, trim, lead)
        assert off[0] == lead != 0 and off[-1] == len(text)
        trimmed = [(it + b";")[:max(len(it) + 1 - trim, 0)] for it in POOL]
        assert trim == 1 or any(len(it) + 1 < trim for it in POOL)
        want = lazy_want(p, trimmed)[idx]
        dev, doff = to_dev(text, off)
        assert dev.untyped_storage().nbytes() == int(off[-1])
        start, end = r.search_extents(dev, doff, trim=trim)
        got = torch.stack([start, end], dim=1).cpu().numpy()
        assert_same(got, want, ("batch", n, trim))
        assert 0 < int((want[:, 1] >= 0).sum()) < n or n == 1


def test_every_alignment_of_item_start_match_end_and_match_start():
    """The same 40-byte item with one match at every offset, each placed at all 16 alignments of its first byte (items of 41 bytes
    with their separator: consecutive copies walk through the 16 residues): the head / wide / tail split of both walks sees a match
    end at address residues 1, 15, 0, 1 ... and the last byte, and match starts on and beside 16-byte boundaries."""
    p = "ab+c"
    items = []
    for needle in (b"abc", b"abbbbbbbbbbbbbbbbbbbc"):              # (the long one: the walk back crosses a 16-byte boundary)
        for at in range(40 - len(needle) + 1):
            it = b"z" * at + needle + b"z" * (40 - at - len(needle))
            assert len(it) == 40
            items += [it] * 16
    want = lazy_want(p, items)
    assert (want[:, 1] >= 0).all() and {int(e) for e in want[:, 1]} >= {3, 15, 16, 17, 40} and {int(s) for s in want[:, 0]} >= {0, 15, 16, 17}
    r = rr.RRegex(p)
    for lead in (0, 3):
        text, offs = pack(items, 1, lead)
        residues = {(int(o), int(o + s) % 16, int(o + e) % 16) for o, (s, e) in zip(offs[:-1] % 16, want)}
        assert len({x[0] for x in residues}) == 16 and len({x[1] for x in residues}) == 16 and len({x[2] for x in residues}) == 16
        dev, doff = to_dev(text, offs)
        assert dev.data_ptr() % 16 == 0
        assert_same(as_pairs(*r.search_extents(dev, doff, trim=1)), want, ("alignment", lead), items)
        # ... and with the byte buffer itself off 16-byte alignment (a slice of a tensor)
        sliced = torch.cat([torch.zeros(5, dtype=torch.uint8, device="cuda"), dev])[5:]
        assert sliced.data_ptr() % 16 == 5
        assert_same(as_pairs(*r.search_extents(sliced, doff, trim=1)), want, ("alignment, sliced", lead), items)


def test_long_items():
    """5 KB ... 100 KB per item, one planted match near the end; a match as long as the pattern allows; a walk back over 30 KB."""
    rng = random.Random(21)
    fill = b"xy zb" * 20001                                         # (no 'a': neither pattern matches inside it)
    for p, needles in (("ab+c", [b"abc", b"abbbbbc", b"a" + b"b" * 30000 + b"c"]), ("a{1,300}", [b"a", b"a" * 1000])):
        items = []
        for k in range(70):
            n = rng.choice([5000, 5001, 20000, 65536, 100000])
            needle = needles[k % len(needles)]
            tail = rng.choice([0, 1, 15, 16, 17, 300])
            it = fill[:max(n - len(needle) - tail, 0)] + needle + fill[:tail]
            items.append(it if k % 9 else fill[:n])                 # one item in nine has no match
        want = lazy_want(p, items)
        assert 0 < int((want[:, 1] < 0).sum()) < len(items) and int(want[:, 1].max()) > 99000
        if p == "a{1,300}":                                         # the smallest end: one byte into the run, wherever the run ends
            found = want[:, 1] >= 0
            assert (want[found, 1] - want[found, 0] == 1).all()
        else:
            assert int((want[:, 1] - want[:, 0]).max()) == 30002
        short = [it[-22:] for it in items]                          # the last 22 bytes: the brute force and the lazy search agree
        assert (want_for(p, short) == lazy_want(p, short)).all()
        r = rr.RRegex(p)
        run_extents(r, items, want, 0, (p, "long, trim 0"))
        run_extents(r, items, want, 1, (p, "long, trim 1"), lead=7)
        run_extents(rr.RRegex(p, rr.ENGINE_DFA_GLOBAL), items, want, 1, (p, "long, global form"))


def test_global_form(reference):
    """RRX_ENGINE_DFA_GLOBAL forces both tables into HBM/L2; under AUTO, a pattern whose two plain tables pass 64 KiB goes there."""
    for p, items, want in reference[:12] + reference[-len(NEWLINE_PATTERNS):]:
        r = rr.RRegex(p, rr.ENGINE_DFA_GLOBAL)
        run_extents(r, items, want, 1, (p[:30], "global form"))
    r = rr.RRegex(GLOBAL_AUTO)
    assert plain_table_bytes(r.program(rr.PROGRAM_SEARCH_FWD)) + plain_table_bytes(r.program(rr.PROGRAM_SEARCH_REV)) > 65536
    rng = random.Random(22)
    items = ["".join(rng.choice("aaabbbx") for _ in range(rng.choice([0, 5, 13, 14, 15, 31, 32, 33, 60]))).encode() for _ in range(300)]
    items += [b"a" + b"b" * 12 + b"x", b"b" * 7 + b"a" + b"ab" * 6 + b"x", b"a" + b"b" * 11 + b"x", b"x" * 20 + b"ab" * 20 + b"x"]
    want = np.array([re_brute_force(GLOBAL_AUTO.encode(), it) for it in items], dtype=np.int32)
    short = [k for k, it in enumerate(items) if len(it) <= 22]
    assert (want_for(GLOBAL_AUTO, [items[k] for k in short]) == want[short]).all()      # (re and the oracle agree where both can tell)
    assert 20 < int((want[:, 1] >= 0).sum()) < len(items)
    run_extents(r, items, want, 0, "AUTO, tables beyond the LDS budget")
    run_extents(r, items, want, 1, "AUTO, tables beyond the LDS budget, trim 1", lead=9)


def test_edge_patterns_and_output_buffers():
    rng = random.Random(23)
    items = short_items(rng, "ab+c", 131)
    text, offs = pack(items, 1, lead=2)
    dev, doff = to_dev(text, offs)
    n = len(items)
    handle = rr.Items(dev, doff, trim=1)

    def poisoned(r, indexed):
        """Both entries through the C ABI on buffers full of 0x5A5A5A5A, one word longer than needed."""
        st = torch.full((n + 1,), POISON, dtype=torch.int32, device="cuda")
        en = torch.full((n + 1,), POISON, dtype=torch.int32, device="cuda")
        stream = rr._stream_ptr(None)
        if indexed:
            rr._check(rr._L.rrx_search_items(r._h, handle._h, st.data_ptr(), en.data_ptr(), stream))
        else:
            rr._check(rr._L.rrx_search_extents(r._h, 0, dev.data_ptr(), doff.data_ptr(), n, 1, st.data_ptr(), en.data_ptr(), stream))
        torch.cuda.synchronize()
        assert int(st[n]) == POISON and int(en[n]) == POISON, "a word behind the results was written"
        got = as_pairs(st[:n], en[:n])
        assert (got != POISON).all(), "a result word was not written"
        return got

    for indexed in (False, True):
        assert_same(poisoned(rr.RRegex("ab+c"), indexed), want_for("ab+c", items), ("poisoned", indexed), items)
        assert (poisoned(rr.RRegex("a*"), indexed) == 0).all()                       # nullable: [0, 0) everywhere, the empty items too
        assert (poisoned(rr.RRegex("[]"), indexed) == -1).all()                      # the empty language
    bad = rr.RRegex(EXPLODING)
    nothing = torch.empty(0, dtype=torch.uint8, device="cuda")
    zero = torch.zeros(1, dtype=torch.int64, device="cuda")
    with pytest.raises(rr.RRegexError, match="determinise"):
        bad.search_extents(dev, doff, trim=1)
    with pytest.raises(rr.RRegexError, match="determinise"):
        bad.search_items(handle)
    with pytest.raises(rr.RRegexError, match="determinise"):
        bad.search_extents(nothing, zero)                                            # ... with zero items as well
    with pytest.raises(rr.RRegexError, match="determinise"):
        bad.search_items(rr.Items(nothing, zero))
    # an empty batch writes nothing
    r = rr.RRegex("ab+c")
    s, e = r.search_extents(nothing, zero)
    assert s.numel() == 0 and e.numel() == 0
    s, e = r.search_items(rr.Items(nothing, zero))
    assert s.numel() == 0 and e.numel() == 0
    # all-empty items: nothing but offsets
    off0 = torch.zeros(70, dtype=torch.int64, device="cuda")
    assert (as_pairs(*r.search_extents(nothing, off0)) == -1).all()
    assert (as_pairs(*rr.RRegex("a*").search_extents(nothing, off0)) == 0).all()
    assert rr._L.rrx_search_extents(r._h, 0, dev.data_ptr(), doff.data_ptr(), 5, 0, None, None, None) == 2      # RRX_ERR_ARG


@pytest.mark.parametrize("kind", ["url", "email", "kwlog"])
def test_search_extents_equals_search_corpus(kind):
    """16 MiB of '\\n' text viewed as items - offsets = the line starts, trim 1: the same (start, end) as rrx_search_corpus."""
    import synth
    pattern = {"url": U2, "email": EMAIL, "kwlog": K1000_CONTAINS}[kind]
    host = synth.corpus(kind, 6, 16 << 20)
    host = host[:int(np.nonzero(host == 10)[0][-1]) + 1]                 # (whole lines: every item has its separator)
    r = rr.RRegex(pattern)
    dev = torch.from_numpy(host).cuda()
    corpus = rr.Corpus(dev)
    ws, we = r.search_corpus(corpus)
    n = corpus.num_lines
    off = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.nonzero(dev == 10).flatten() + 1]).contiguous()
    assert off.numel() == n + 1
    found = int((we >= 0).sum())
    assert 0 < found and (kind == "kwlog" or found < n)
    gs, ge = r.search_extents(dev, off, trim=1)
    assert torch.equal(ge, we), (kind, "end", int(torch.nonzero(ge != we)[0]))
    assert torch.equal(gs, ws), (kind, "start", int(torch.nonzero(gs != ws)[0]))
    gs, ge = r.search_items(rr.Items(dev, off, trim=1))
    assert torch.equal(ge, we) and torch.equal(gs, ws), (kind, "indexed")


def test_a_side_stream_and_a_captured_graph(reference):
    p, items, want = next(x for x in reference if x[0] == EMAIL)
    r = rr.RRegex(p)
    text, offs = pack(items, 1, lead=1)
    dev, doff = to_dev(text, offs)
    n = len(items)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    s, e = r.search_extents(dev, doff, trim=1, stream=side)
    side.synchronize()
    assert_same(as_pairs(s, e), want, "side stream", items)
    # one call captured (the tables are up: nothing is allocated or uploaded inside the capture), replayed on refilled inputs
    st = torch.full((n,), POISON, dtype=torch.int32, device="cuda")
    en = torch.full((n,), POISON, dtype=torch.int32, device="cuda")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            rr._check(rr._L.rrx_search_extents(r._h, 0, dev.data_ptr(), doff.data_ptr(), n, 1, st.data_ptr(), en.data_ptr(), rr._stream_ptr(side)))
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
        assert_same(as_pairs(*r.search_extents(dev, doff, trim=1)), want[order], ("direct call", round_), shuffled)
