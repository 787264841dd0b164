"""rrx_contains_extents / rrx_contains_items on the device: bit i = item i contains a match.  Against the oracle's brute force on
short items and Python's re (on patterns whose semantics the dialects share) on long ones, on every route - an indexed batch on
the byte-stride and the stride-2 items kernels, the one-call form below and above the stripe-wise thresholds, fit and unfit, the
lane-per-item kernel on an LDS and on a global table - and against rrx_contains_corpus word for word at scale."""
import random
import re

import numpy as np
import pytest

import roaringregex_amd as rr
from contains_cases import EXPLODING, unpack
from patterns import EMAIL, K1000, K1000_CONTAINS, U2
from test_contains_items_lowering import NEWLINE_PATTERNS, short_items, want_for

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

# pattern -> (Python re of the same language on bytes, alphabet of the random text, a match to plant)
CASES = {
    "ab+c": (rb"ab+c", b"abc xyz\n", b"abbc"),
    EMAIL: (EMAIL.encode(), b"ab1._@ Z\n", b"a.b@c1"),
    "a\nb": (rb"a\nb", b"ab\n cd", b"a\nb"),
    U2: (U2.encode(), b"ab1.:/htps \n", b"http://ab.ba/a1"),
}
DIRT = (b"\x00", b"\x80", b"\xff", b"\xc3\xa9", b"\n")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"


def pack(items, trim, rng=None, lead=0):
    """items -> (text, offsets): every item followed by `trim` separator bytes of any value, `lead` bytes in front of the first."""
    seps = b"ab\n;\x00\xff"
    parts, offs, at = [b"q" * lead], [lead], lead
    for it in items:
        sep = bytes(seps[rng.randrange(len(seps))] for _ in range(trim)) if trim else b""
        parts.append(it + sep)
        at += len(it) + trim
        offs.append(at)
    text = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
    return text, np.array(offs, dtype=np.int64)


def to_dev(text, offs):
    d = torch.from_numpy(text).cuda() if len(text) else torch.empty(0, dtype=torch.uint8, device="cuda")
    return d, torch.from_numpy(offs).cuda()


def want_re(rx, items):
    c = re.compile(rx)
    return np.array([1 if c.search(it) else 0 for it in items], dtype=np.uint8)


def batch(seed, p, n, lens, probs):
    """n random items: lengths from `lens`, one in four with a match planted (at the start, at the end or inside), one in nine with
    a NUL, a high byte or a '\\n' somewhere; then the fixed geometry cases."""
    rx, alphabet, needle = CASES[p]
    rng = np.random.default_rng(seed)
    prng = random.Random(seed)
    a = np.frombuffer(alphabet, dtype=np.uint8)
    items = []
    for L in rng.choice(lens, size=n, p=probs):
        it = bytearray(a[rng.integers(0, len(a), size=int(L))].tobytes())
        k = prng.randrange(36)
        if k < 9 and L >= len(needle):
            at = 0 if k < 2 else L - len(needle) if k < 4 else prng.randrange(L - len(needle) + 1)
            it[at:at + len(needle)] = needle
        if k % 9 == 4 and L:
            d = prng.choice(DIRT)
            at = prng.randrange(L)
            it[at:at + len(d)] = d
            del it[int(L):]
        items.append(bytes(it))
    half = len(needle) // 2
    fill = (b"xy z" * 10001)
    items += [needle[:half], needle[half:], needle[:half], needle[half:],            # a would-be match across two items: not found
              needle, b"z" + needle, needle + b"z", needle[:1], needle[-1:], needle[:2], needle[:3],
              needle + fill[:40000], fill[:40000] + needle, fill[:40000], fill[:20000] + needle + fill[:20000], fill[:39999] + needle[:half], needle[half:],
              b"\xff" + needle + b"\x00", b"\n" + needle + b"\n"]
    return items, want_re(rx, items)


def check_bits(r, bits, n, want, what):
    got = unpack(bits.cpu().numpy(), n)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (what, r.pattern[:30], "first bad item", int(bad[0]), int(got[bad[0]]))
    assert rr.bitmap_count(bits, n) == int(want.sum()), what
    if n & 31:
        assert (int(bits[-1].item()) & 0xffffffff) >> (n & 31) == 0, (what, "bits beyond the last item")


def run_indexed(r, items, want, trim, rng, what, expect_stripes=True, lead=0):
    text, offs = pack(items, trim, rng, lead)
    dev, doff = to_dev(text, offs)
    handle = rr.Items(dev, doff, trim=trim)
    assert handle.stripe_wise == expect_stripes, what
    bits = r.contains_items_bits(handle)
    check_bits(r, bits, len(items), want, what)
    by_byte = r.contains_items(handle).cpu().numpy()
    assert (by_byte == want).all(), what


def run_extents(r, items, want, trim, rng, what, lead=0):
    text, offs = pack(items, trim, rng, lead)
    dev, doff = to_dev(text, offs)
    bits = r.contains_extents_bits(dev, doff, trim=trim)
    check_bits(r, bits, len(items), want, what)
    by_byte = r.contains_extents(dev, doff, trim=trim).cpu().numpy()
    assert (by_byte == want).all(), what


LENS, PROBS = [1, 2, 3, 7, 19, 64, 300, 5000, 40_000], [0.15, 0.15, 0.15, 0.2, 0.2, 0.1, 0.04, 0.009, 0.001]


def test_indexed_batches_against_the_oracle():
    """rr.Items: the byte-stride items kernel (trim 0; trim 1 with the stride-2 form switched off) and the stride-2 items kernel (trim 1)
    on the contains items tables; U2 has none and runs a lane per item on its LDS table."""
    rng = random.Random(11)
    for seed, p in enumerate(CASES):
        items, want = batch(100 + seed, p, 6000, LENS, PROBS)
        assert 0 < want.sum() < len(want)
        r = rr.RRegex(p)
        has_forms = r.program(rr.PROGRAM_CONTAINS_DFA2_ITEMS) is not None
        assert has_forms == (p != U2)
        for trim in (0, 1):
            run_indexed(r, items, want, trim, rng, "indexed trim %d" % trim)
        r.set_items_stride2(False)
        run_indexed(r, items, want, 1, rng, "indexed trim 1, byte stride")
        forced = rr.RRegex(p, rr.ENGINE_DFA)                            # (a regex that stays on byte-stride forms)
        run_indexed(forced, items, want, 1, rng, "indexed trim 1, RRX_ENGINE_DFA")


def test_short_items_against_the_brute_force():
    """The CPU test's items and ground truth (brute force over substrings with the oracle's acceptance) on the device: a small
    one-call batch (a lane per item - on an LDS table, and on a global table under RRX_ENGINE_DFA_GLOBAL), an indexed batch with
    separators (stripe-wise), and an indexed batch without (its empty items make it unfit: a lane per item)."""
    rng = random.Random(12)
    for p in ["ab+c", "a*", "(a|b)*abb", "k(1|10|100)", EMAIL, U2, K1000] + NEWLINE_PATTERNS:
        items = short_items(rng, p, 240)
        want = want_for(p, items)
        for e in (rr.ENGINE_AUTO, rr.ENGINE_DFA_GLOBAL, rr.ENGINE_NFA):
            try:
                r = rr.RRegex(p, e)
            except rr.RRegexError:
                assert e == rr.ENGINE_NFA                                  # (no NFA lane program for this pattern: nothing to show)
                continue
            for trim in (0, 1, 2):
                run_extents(r, items, want, trim, rng, "small one-call trim %d engine %d" % (trim, e))
            run_indexed(r, items, want, 1, rng, "indexed short trim 1")
            run_indexed(r, items, want, 0, rng, "indexed short trim 0 (empty items)", expect_stripes=False)
            run_indexed(r, items, want, 2, rng, "indexed short trim 2", expect_stripes=False)


BIG_LENS, BIG_PROBS = [1, 2, 3, 40, 120, 200, 400], [0.05, 0.05, 0.05, 0.15, 0.3, 0.25, 0.15]


def test_large_one_call_batches():
    """>= 65536 items and >= 8 MiB: the one-call stripe-wise route (index, stripe-wise kernel, copy, predicated fallback) - and the
    same batch made unfit (a start off 16-byte alignment, trim 2, an empty item at trim 0): the fallback answers, exactly."""
    rng = random.Random(13)
    for seed, p in enumerate(("ab+c", EMAIL, "a\nb", U2)):
        items, want = batch(200 + seed, p, 70_000, BIG_LENS, BIG_PROBS)
        assert len(items) >= 65536 and sum(len(it) for it in items) >= (8 << 20) and len(items) % 32
        assert 0 < want.sum() < len(want)
        r = rr.RRegex(p)
        for trim in (0, 1):
            run_extents(r, items, want, trim, rng, "large trim %d" % trim)
        if p == EMAIL:
            r.set_items_stride2(False)
            run_extents(r, items, want, 1, rng, "large trim 1, byte stride")
            run_extents(rr.RRegex(p, rr.ENGINE_DFA_GLOBAL), items, want, 1, rng, "large trim 1, RRX_ENGINE_DFA_GLOBAL")
        if p in ("ab+c", U2):
            run_extents(r, items, want, 1, rng, "large, misaligned start", lead=3)
            run_extents(r, items, want, 2, rng, "large, trim 2")
            holed = items[:1000] + [b""] + items[1000:]
            run_extents(r, holed, np.insert(want, 1000, 0), 0, rng, "large, an empty item at trim 0")
            run_indexed(r, items, want, 1, rng, "indexed, misaligned start", expect_stripes=False, lead=3)
    # the nullable pattern: every item, the empty one of an unfit batch included
    items, _ = batch(299, "ab+c", 70_000, BIG_LENS, BIG_PROBS)
    items[777] = b""
    r = rr.RRegex("a*")
    for trim in (0, 1):
        run_extents(r, items, np.ones(len(items), dtype=np.uint8), trim, rng, "nullable, large trim %d" % trim)
    run_extents(rr.RRegex("[]"), items, np.zeros(len(items), dtype=np.uint8), 1, rng, "empty language, large")


def sprinkle_utf8(host, seed):
    """A two-byte UTF-8 character over two text bytes at about one line in a hundred (never over a '\\n')."""
    rng = np.random.default_rng(seed)
    out = host.copy()
    nlines = int((host == 10).sum())
    pos = rng.integers(0, host.size - 1, size=max(nlines // 100, 1))
    pos = pos[(host[pos] != 10) & (host[pos + 1] != 10)]
    out[pos] = 0xC3
    out[pos + 1] = 0xA9
    return out


@pytest.mark.parametrize("kind", ["url", "email", "kwlog"])
def test_contains_items_equals_contains_corpus_at_scale(kind):
    """A 256 MiB '\\n' corpus viewed as items - offsets = the line starts, trim 1: the two entries must give the same bitmap."""
    import synth
    pattern = {"url": U2, "email": EMAIL, "kwlog": K1000_CONTAINS}[kind]
    host = sprinkle_utf8(synth.corpus(kind, 6, 256 << 20), 3)
    host = host[:int(np.nonzero(host == 10)[0][-1]) + 1]                 # (whole lines: every item has its separator)
    r = rr.RRegex(pattern)
    dev = torch.from_numpy(host).cuda()
    corpus = rr.Corpus(dev)
    want = r.contains_corpus_bits(corpus).clone()
    n = corpus.num_lines
    off = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.nonzero(dev == 10).flatten() + 1]).contiguous()
    assert off.numel() == n + 1
    popcount = int(unpack(want.cpu().numpy(), n).sum())
    assert 0 < popcount < n
    items = rr.Items(dev, off, trim=1)
    assert items.stripe_wise
    got = r.contains_items_bits(items)
    assert torch.equal(got, want), (kind, "indexed", int(torch.nonzero(got != want)[0]))
    assert rr.bitmap_count(got, n) == popcount
    got = r.contains_extents_bits(dev, off, trim=1)
    assert torch.equal(got, want), (kind, "one call", int(torch.nonzero(got != want)[0]))
    assert rr.bitmap_count(got, n) == popcount


def test_bitmap_hygiene():
    """nitems off a multiple of 32, `out` full of ones and longer than needed: the bits of the last word beyond nitems come back 0,
    the words behind it are not touched - on every route."""
    rng = random.Random(14)
    small, want_small = batch(301, EMAIL, 1000, [1, 7, 19, 64], [0.25, 0.25, 0.25, 0.25])
    big, want_big = batch(302, EMAIL, 70_000, BIG_LENS, BIG_PROBS)
    r = rr.RRegex(EMAIL)
    for items, want, trim, lead in ((small, want_small, 0, 0), (small, want_small, 1, 0), (big, want_big, 1, 0), (big, want_big, 0, 0), (big, want_big, 1, 5)):
        n = len(items)
        assert n % 32
        nw = (n + 31) // 32
        text, offs = pack(items, trim, rng, lead)
        dev, doff = to_dev(text, offs)
        handle = rr.Items(dev, doff, trim=trim)
        for route in ("one call", "indexed"):
            out = torch.full((nw + 9,), -1, dtype=torch.int32, device="cuda")
            bits = r.contains_extents_bits(dev, doff, trim=trim, out=out) if route == "one call" else r.contains_items_bits(handle, out=out)
            assert bits.numel() == nw
            check_bits(r, bits, n, want, (route, n, trim, lead))
            assert (out[nw:] == -1).all(), (route, n, trim, lead, "words behind the bitmap were written")


def test_two_streams_share_the_scratch_in_order():
    """Two regexes, two batches alternating on two streams, no host synchronisation in between: the one-call form's index and result
    scratch belong to the regex and are handed from stream to stream by an event - every result must be its own batch's."""
    import synth
    regs = [rr.RRegex(EMAIL), rr.RRegex("[0-9]+\\.[a-z]+")]
    batches = []
    for seed in (31, 32):
        host = sprinkle_utf8(synth.corpus("email", seed, 24 << 20), seed)
        host = host[:int(np.nonzero(host == 10)[0][-1]) + 1]
        dev = torch.from_numpy(host).cuda()
        off = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.nonzero(dev == 10).flatten() + 1]).contiguous()
        corpus = rr.Corpus(dev)
        want = [r.contains_corpus_bits(corpus).clone() for r in regs]
        batches.append((dev, off, want))
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [[[torch.empty_like(b[2][j]) for _ in range(4)] for j in range(2)] for b in batches]
    for it in range(4):
        for k in (0, 1):
            dev, off, _ = batches[k]
            for j, r in enumerate(regs):
                r.contains_extents_bits(dev, off, trim=1, out=outs[k][j][it], stream=streams[k])
    torch.cuda.synchronize()
    for k in (0, 1):
        for j in (0, 1):
            assert 0 < int(unpack(batches[k][2][j].cpu().numpy(), batches[k][1].numel() - 1).sum())
            for it in range(4):
                assert torch.equal(outs[k][j][it], batches[k][2][j]), (k, j, it)


def test_an_indexed_launch_is_captured_and_replayed():
    rng = random.Random(15)
    items, want = batch(303, EMAIL, 6000, LENS, PROBS)
    text, offs = pack(items, 1, rng)
    dev, doff = to_dev(text, offs)
    handle = rr.Items(dev, doff, trim=1)
    r = rr.RRegex(EMAIL)
    eager = r.contains_items_bits(handle).clone()
    check_bits(r, eager, len(items), want, "eager")
    out = torch.zeros_like(eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        r.contains_items_bits(handle, out=out)                         # (tables are up, nothing is allocated inside the capture)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            r.contains_items_bits(handle, out=out)
    torch.cuda.current_stream().wait_stream(side)
    out.fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_degenerate_inputs():
    r = rr.RRegex("ab?")
    nothing = torch.empty(0, dtype=torch.uint8, device="cuda")
    zero = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert r.contains_extents_bits(nothing, zero).numel() == 0 and r.contains_extents(nothing, zero).numel() == 0
    handle = rr.Items(nothing, zero)
    assert r.contains_items_bits(handle).numel() == 0 and r.contains_items(handle).numel() == 0
    # all-empty items: trim 0 (nothing but offsets) and trim 1 (nothing but separators)
    for p, verdict in (("ab?", 0), ("a*", 1), ("[]", 0)):
        r = rr.RRegex(p)
        for n in (1, 33, 70_001):
            want = np.full(n, verdict, dtype=np.uint8)
            off0 = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
            check_bits(r, r.contains_extents_bits(torch.zeros(16, dtype=torch.uint8, device="cuda"), off0), n, want, ("all empty, trim 0", n))
            seps = torch.full((n,), ord("a"), dtype=torch.uint8, device="cuda")
            off1 = torch.arange(n + 1, dtype=torch.int64, device="cuda")
            check_bits(r, r.contains_extents_bits(seps, off1, trim=1), n, want, ("all empty, trim 1", n))
            check_bits(r, r.contains_items_bits(rr.Items(seps, off1, trim=1)), n, want, ("all empty, indexed trim 1", n))
    bad = rr.RRegex(EXPLODING)
    items, _ = batch(304, "ab+c", 100, [7], [1.0])
    dev, doff = to_dev(*pack(items, 0))
    with pytest.raises(rr.RRegexError, match="contains"):
        bad.contains_extents_bits(dev, doff)
    with pytest.raises(rr.RRegexError, match="contains"):
        bad.contains_items_bits(rr.Items(dev, doff))
    r = rr.RRegex("a")
    assert rr._L.rrx_contains_extents(None, 0, None, None, 0, 0, None, None) == 2
    assert rr._L.rrx_contains_extents(r._h, 0, dev.data_ptr(), doff.data_ptr(), 5, 0, None, None) == 2     # RRX_ERR_ARG: no bitmap for a batch with items
    assert rr._L.rrx_contains_items(r._h, None, None, None) == 2


MATCH_GLOBAL = "[ab]*a[ab]{12}c"                    # 8194 states of 4 classes: its plain match table passes 64 KiB and stays in HBM/L2


def test_every_alignment_of_item_start_on_the_lane_kernels():
    """match_extents_kernel and contains_extents_kernel: items of every length 0 ... 40, each placed at all 16 alignments of its first
    byte, trim 1 - on a 16-byte aligned buffer and on the same buffer sliced by one byte (both kernels align on the OFFSET, so on the
    slice every wide load is an unaligned one), tables in LDS and in HBM/L2.  One round of the 41 lengths takes 861 bytes, 13 mod 16:
    16 rounds carry every length through the 16 residues.  656 items: far below the stripe-wise thresholds, a lane per item.
    Expected: the oracle's whole-string acceptance (match) and its brute-force search (contains)."""
    from contains_cases import brute_force
    from pyoracle import OracleRegex
    from table_edge_cases import plain_table_bytes
    rng = random.Random(31)
    small = ("ab+c", "abcz", 3, lambda n: b"a" + b"b" * (n - 2) + b"c")
    large = (MATCH_GLOBAL, "abc", 14, lambda n: b"b" * (n - 14) + b"a" + b"b" * 12 + b"c")
    # (pattern ..., engine, match on the lane kernel's LDS / global form, contains on its LDS / global form or None)
    for (p, alphabet, shortest, witness), engine, match_form, contains_form in ((small, rr.ENGINE_AUTO, "lds", "lds"), (small, rr.ENGINE_DFA_GLOBAL, "lds", "global"),
                                                                                (large, rr.ENGINE_DFA_GLOBAL, "global", None)):
        items = []
        for _ in range(16):
            for n in range(41):
                it = "".join(rng.choice(alphabet) for _ in range(n)).encode()
                k = rng.randrange(4)
                if k == 0 and n >= shortest:
                    it = witness(n)                                                         # the whole item matches
                elif k == 1 and n >= shortest:
                    at = rng.randrange(n - shortest + 1)
                    it = it[:at] + witness(shortest) + it[at + shortest:]                  # a match somewhere inside
                items.append(it)
        o = OracleRegex(p)
        want_match = np.array([1 if o.accepts(it) else 0 for it in items], dtype=np.uint8)
        assert len(items) == 656 and 50 < want_match.sum() < 400
        text, offs = pack(items, 1, rng)
        assert len({(int(at) % 16, len(it)) for at, it in zip(offs[:-1], items)}) == 16 * 41
        dev, doff = to_dev(text, offs)
        sliced = torch.cat([torch.zeros(1, dtype=torch.uint8, device="cuda"), dev])[1:]
        assert dev.data_ptr() % 16 == 0 and sliced.data_ptr() % 16 == 1
        r = rr.RRegex(p, engine)
        assert r.engine_name.startswith("dfa"), r.engine_name                               # (match_extents on the plain table)
        assert (plain_table_bytes(r.program(rr.ENGINE_DFA)) > 65536) == (match_form == "global")
        for buf, what in ((dev, "aligned"), (sliced, "sliced by one byte")):
            got = r.match_extents(buf, doff, trim=1).cpu().numpy()
            bad = np.nonzero(got != want_match)[0]
            assert bad.size == 0, ("match", p, match_form, what, int(bad[0]), items[bad[0]], int(offs[bad[0]]) % 16)
        if contains_form:
            want_contains = brute_force(p, b"\n".join(items) + b"\n")
            assert want_match.sum() < want_contains.sum() < len(items)
            assert plain_table_bytes(r.program(rr.PROGRAM_CONTAINS_DFA)) <= 65536           # (global only because the regex asked for it)
            for buf, what in ((dev, "aligned"), (sliced, "sliced by one byte")):
                check_bits(r, r.contains_extents_bits(buf, doff, trim=1), len(items), want_contains, ("contains", p, contains_form, what))
