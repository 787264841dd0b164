"""Contains on the NFA lane engine (RRX_OPT_CONTAINS_NFA) on the device: ContainsLineNfaEngine<W, RULES> behind rrx_contains_corpus
and contains_extents_nfa_kernel<W> behind rrx_contains_extents / rrx_contains_items (kernels_nfa.inc), against the expectations of
contains_nfa_cases.py - the vectors test_contains_nfa_lowering.py holds the replay of the same program to, where the cases are shown
to reach all 16 line kernels and all 8 items kernels."""
import random
import re

import numpy as np
import pytest
import torch

import contains_cases as CC
import contains_nfa_cases as T
import roaringregex_amd as rr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"


def nfa_regex(pattern, mode=2):
    r = rr.RRegex(pattern)
    r.set_contains_nfa(mode)
    return r


def dev(data):
    return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda() if len(data) else torch.empty(0, dtype=torch.uint8, device="cuda")


def check_bits(bits, n, want, what):
    got = T.unpack(bits.cpu().numpy(), n)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, "first bad", int(bad[0]), "got", int(got[bad[0]]), "of", n)
    assert rr.bitmap_count(bits, n) == int(want.sum()), what
    if n & 31:
        assert (int(bits[-1].item()) & 0xffffffff) >> (n & 31) == 0, (what, "bits beyond the last one")


def check_corpus(r, data, want, what, stripes=(512, 1024, 0)):
    for stripe in stripes:
        c = rr.Corpus(dev(data), stripe=stripe)
        assert c.num_lines == len(want), (what, stripe)
        check_bits(r.contains_corpus_bits(c), len(want), want, (what, "stripe", stripe))


def pack(lines, trim):
    off = np.zeros(len(lines) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(t) + trim for t in lines])
    return b"".join(t + b";" * trim for t in lines), off


def check_items(r, lines, want, what):
    """contains_extents_bits at trim 0 and trim 1, contains_items_bits on an rr.Items (trim 1)"""
    for trim in (0, 1):
        data, off = pack(lines, trim)
        d, o = dev(data if data else b"\x00"), torch.from_numpy(off).cuda()
        check_bits(r.contains_extents_bits(d, o, trim=trim), len(lines), want, (what, "extents, trim", trim))
    check_bits(r.contains_items_bits(rr.Items(d, o, trim=1)), len(lines), want, (what, "items, trim 1"))


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id)
def test_every_case_under_option_2(case):
    r = nfa_regex(case.pattern)
    assert r.contains_engine_name == "nfa-shift-and"
    lines, want = T.build(case)
    check_corpus(r, T.corpus(case), want, "final newline")
    check_corpus(r, T.corpus(case, final_newline=False), want, "no final newline")
    check_items(r, lines, want, case.id)


@pytest.mark.parametrize("pattern", T.TABLELESS)
def test_the_tableless_patterns_under_option_1(pattern):
    r = nfa_regex(pattern, mode=1)
    assert r.contains_engine_name == "nfa-shift-and" and r.contains_states == 0
    lines, want = T.tableless_lines(pattern), T.tableless_expected(pattern)
    data = b"\n".join(lines) + b"\n"
    check_corpus(r, data, want, pattern)
    check_items(r, lines, want, pattern)
    r.set_contains_nfa(0)                                  # the same regex, the option back at its default: no table, as ever
    c = rr.Corpus(dev(data))
    d, o = dev(data), torch.from_numpy(pack(lines, 1)[1]).cuda()
    for call in (lambda: r.contains_corpus_bits(c), lambda: r.contains_extents_bits(d, o, trim=1), lambda: r.contains_items_bits(rr.Items(d, o, trim=1))):
        with pytest.raises(rr.RRegexError, match="determinise"):
            call()


def test_tableless_14_short_lines_with_nul_and_high_bytes():
    p = T.TABLELESS[0]
    rng = random.Random(14)
    lines = []
    for _ in range(400):
        t = bytearray("".join(rng.choice("aab") for _ in range(rng.choice((0, 3, 14, 15, 16, 20, 22)))).encode())
        if t and rng.random() < 0.3:
            t[rng.randrange(len(t))] = rng.choice((0, 0x80, 0xff, ord("-")))
        lines.append(bytes(t))
    lines.append(b"b")
    data = b"\n".join(lines) + b"\n"
    want = CC.brute_force(p, np.frombuffer(data, dtype=np.uint8))
    r = nfa_regex(p, mode=1)
    check_corpus(r, data, want, "short lines")
    check_items(r, lines, want, "short lines")


# ---- edges
def test_corpus_edges():
    r = nfa_regex("ab+c")
    hit, miss = b"zabbc", b"zabbz"
    # a line that starts exactly at a stripe boundary (512): the line before it ends on byte 511
    first = b"k" * 511
    check_corpus(r, first + b"\n" + b"abc\n" + b"ab\n", np.array([0, 1, 0], dtype=np.uint8), "line at a stripe boundary", stripes=(512,))
    # a line longer than a stripe whose only match lies past the stripe end: the follow-on walk (and a lane that starts inside it)
    long_line = b"ab" * 300 + b"abbbc" + b"ab" * 400
    data = b"zz\n" + long_line + b"\nabc\n" + b"ab" * 700 + b"\n"
    check_corpus(r, data, np.array([0, 1, 1, 0], dtype=np.uint8), "match past the stripe end", stripes=(512, 1024))
    # a match that ends on the byte before '\n', a match at the very first byte of the corpus, no match across a '\n'
    check_corpus(r, b"abc\nzzabc\nab\nc\nabbbbc", np.array([1, 1, 0, 0, 1], dtype=np.uint8), "first byte, last byte, across a newline")
    # one line without '\n', with and without a match; an empty line between others; a NUL and a high byte in front of a match
    check_corpus(r, hit, np.array([1], dtype=np.uint8), "one line, no newline")
    check_corpus(r, miss, np.array([0], dtype=np.uint8), "one line, no newline, no match")
    check_corpus(r, b"abc\n\n\nabc\n\x00abc\n\xc3\xa9abc\nab\x00c\n", np.array([1, 0, 0, 1, 1, 1, 0], dtype=np.uint8), "empty lines, NUL, high bytes")
    # more than one workgroup at 512-byte stripes: 1024 lanes of 512 bytes each, and a little more
    rng = random.Random(5)
    lines = [bytes(rng.choice(b"abcz") for _ in range(rng.choice((0, 5, 40, 200)))) for _ in range(9000)]
    want = np.array([1 if re.search(rb"ab+c", t) else 0 for t in lines], dtype=np.uint8)
    data = b"\n".join(lines) + b"\n"
    assert len(data) > 1024 * 512 + 4096
    check_corpus(r, data, want, "two workgroups", stripes=(512, 0))


def test_items_edges():
    r = nfa_regex("ab+c")
    check_items(r, [b"", b"abc", b"", b"ab", b"zzabbbc", b"\x00abc", b"ab\xffc"], np.array([0, 1, 0, 0, 1, 1, 0], dtype=np.uint8), "empty items")
    nl = nfa_regex("a\nb")                                 # '\n' inside an item as part of a match
    check_items(nl, [b"a\nb", b"za\nbz", b"a\n", b"\nb", b"a\n\nb", b"ab"], np.array([1, 1, 0, 0, 0, 0], dtype=np.uint8), "newline in a match")
    # 70 001 items: 69 workgroups, the last ballot covers 49 items, the last word is partial
    n = 70_001
    rng = np.random.default_rng(70001)
    lens = rng.integers(0, 9, size=n)
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens + 1)
    text = np.frombuffer(b"abcz", dtype=np.uint8)[rng.integers(0, 4, size=int(off[-1]))]
    hostb = text.tobytes()
    rx = re.compile(rb"ab+c")
    want = np.array([1 if rx.search(hostb[off[i]:off[i + 1] - 1]) else 0 for i in range(n)], dtype=np.uint8)
    d, o = torch.from_numpy(text.copy()).cuda(), torch.from_numpy(off).cuda()
    check_bits(r.contains_extents_bits(d, o, trim=1), n, want, "70 001 items")
    check_bits(r.contains_items_bits(rr.Items(d, o, trim=1)), n, want, "70 001 indexed items")


def test_the_grid_strides_beyond_2_20_items():
    """the items launch is bounded at 1024 workgroups of 1024 lanes: the items behind 2^20 are a workgroup's second pass"""
    n = (1 << 20) + 70_001
    rng = np.random.default_rng(20)
    text = np.frombuffer(b"abc", dtype=np.uint8)[rng.integers(0, 3, size=4 * n)]
    off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * 4
    t4 = text.reshape(n, 4)
    a, b, c = ord("a"), ord("b"), ord("c")
    want = (((t4[:, 0] == a) & (t4[:, 1] == b) & ((t4[:, 2] == c) | ((t4[:, 2] == b) & (t4[:, 3] == c)))) |
            ((t4[:, 1] == a) & (t4[:, 2] == b) & (t4[:, 3] == c))).astype(np.uint8)
    r = nfa_regex("ab+c")
    check_bits(r.contains_extents_bits(torch.from_numpy(text.copy()).cuda(), off), n, want, "2^20 + 70 001 items")


def test_every_alignment_of_item_start():
    """items of every length 0 ... 40 at all 16 alignments of their first byte (the pattern of
    test_every_alignment_of_item_start_on_the_lane_kernels), on an aligned buffer and on the same buffer sliced by one byte"""
    rng = random.Random(31)
    items = []
    for _ in range(16):
        for n in range(41):
            it = "".join(rng.choice("abcz") for _ in range(n)).encode()
            k = rng.randrange(4)
            if k == 0 and n >= 3:
                it = b"a" + b"b" * (n - 2) + b"c"
            elif k == 1 and n >= 3:
                at = rng.randrange(n - 2)
                it = it[:at] + b"abc" + it[at + 3:]
            items.append(it)
    data = b"\n".join(items) + b"\n"
    want = CC.brute_force("ab+c", np.frombuffer(data, dtype=np.uint8))
    assert len(want) == len(items) == 656 and 50 < want.sum() < 500
    text, off = pack(items, 1)
    assert len({(int(at) % 16, len(it)) for at, it in zip(off[:-1], items)}) == 16 * 41
    d, o = dev(text), torch.from_numpy(off).cuda()
    sliced = torch.cat([torch.zeros(1, dtype=torch.uint8, device="cuda"), d])[1:]
    assert d.data_ptr() % 16 == 0 and sliced.data_ptr() % 16 == 1
    r = nfa_regex("ab+c")
    for buf in (d, sliced):
        check_bits(r.contains_extents_bits(buf, o, trim=1), len(items), want, "alignment")


def test_nullable_and_empty_language():
    data = b"abc\n\nzz\x00\n" * 23 + b"tail"
    lines = CC.split_lines(data)
    for p, verdict in (("a*", 1), ("[]", 0)):
        r = nfa_regex(p)
        want = np.full(len(lines), verdict, dtype=np.uint8)
        check_corpus(r, data, want, p)
        check_items(r, lines, want, p)
        for n in (1, 32, 33):
            check_items(r, lines[:n], want[:n], (p, n))
    r = nfa_regex("a*")
    nothing, zero = torch.empty(0, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    assert r.contains_extents_bits(nothing, zero).numel() == 0 and r.contains_corpus_bits(rr.Corpus(nothing)).numel() == 0


@pytest.mark.parametrize("pattern", CC.FIXED, ids=lambda p: p[:20])
def test_nfa_equals_the_table(pattern):
    """where a table exists, option 2 equals option 0 on the 3000 short lines with NUL and high bytes"""
    lines = CC.short_lines(random.Random(pattern), pattern, 3000)
    lines[-1] = lines[-1] or b"a"
    data = b"\n".join(lines) + b"\n"
    table, nfa = rr.RRegex(pattern), nfa_regex(pattern)
    assert table.contains_engine_name.startswith("dfa-") and nfa.contains_engine_name == "nfa-shift-and"
    c = rr.Corpus(dev(data))
    want = T.unpack(table.contains_corpus_bits(c).cpu().numpy(), len(lines))
    check_corpus(nfa, data, want, pattern, stripes=(512, 0))
    check_items(nfa, lines, want, pattern)


def test_one_capture_under_option_1():
    p = CC.EXPLODING
    lines, want = T.tableless_lines(p), T.tableless_expected(p)
    c = rr.Corpus(dev(b"\n".join(lines) + b"\n"))
    r = nfa_regex(p, mode=1)
    eager = r.contains_corpus_bits(c).clone()              # (the warm-up call: the program is uploaded here)
    check_bits(eager, len(lines), want, "eager")
    out = torch.zeros_like(eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            r.contains_corpus_bits(c, out=out)
    torch.cuda.current_stream().wait_stream(side)
    out.fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
