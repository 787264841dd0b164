"""rrx_contains_corpus on the device: bit i = line i contains a match = rrx_search_corpus reports one for it.  Against the oracle
(brute-force search on short lines, its own automaton of .*(p).* on ASCII lines), against rrx_search_corpus at scale, on every
table form (stride-2 with and without bytes >= 0x80 in the corpus, wide / classed LDS table, global table), and rrx_bitmap_count."""
import random
import re

import numpy as np
import pytest

import roaringregex_amd as rr
from contains_cases import (brute_force, dot_star, long_ascii_lines, short_line_patterns, short_lines, split_lines, unpack)
from patterns import EMAIL, K1000_CONTAINS, U2

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FORMS = (rr.ENGINE_AUTO, rr.ENGINE_DFA, rr.ENGINE_DFA_GLOBAL)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"


def to_dev(data):
    a = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data
    return torch.from_numpy(np.array(a, copy=True)).cuda() if len(a) else torch.empty(0, dtype=torch.uint8, device="cuda")


def contains(r, data, stripe=0):
    corpus = rr.Corpus(to_dev(data), stripe=stripe)
    bits = r.contains_corpus_bits(corpus)
    got = unpack(bits.cpu().numpy(), corpus.num_lines)
    by_byte = r.contains_corpus(corpus).cpu().numpy()
    assert got.shape == by_byte.shape and (got == by_byte).all()
    assert rr.bitmap_count(bits, corpus.num_lines) == int(got.sum())
    return got


def check(r, data, want, stripes=(0,), what=""):
    for stripe in stripes:
        got = contains(r, data, stripe)
        assert got.shape == want.shape, (what, r.pattern[:40], stripe, got.shape, want.shape)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (what, r.pattern[:40], r.contains_engine_name, "stripe", stripe, "line", int(bad[0]), split_lines(data)[bad[0]][:60], int(got[bad[0]]))


def test_contains_against_the_oracle():
    """Short lines with NUL and high bytes against the brute-force search; the same text with every high byte and NUL replaced by a
    space (a corpus without bytes >= 0x80: the plain stride-2 kernel) too; long ASCII lines against the oracle's .*(p).*."""
    rng = random.Random(881)
    for p in short_line_patterns() + ["a*", EMAIL, U2]:
        r = rr.RRegex(p)
        lines = short_lines(rng, p, 3000)
        ascii_lines = [bytes(32 if c >= 0x80 else c for c in ln) for ln in lines]
        for tail in (b"\n", b""):
            for ls in (lines, ascii_lines):
                data = b"\n".join(ls) + tail
                check(r, data, brute_force(p, data), stripes=(512, 1024, 4096, 0), what="short")
    for p in short_line_patterns()[:12] + [EMAIL, U2, K1000_CONTAINS, "a*"]:
        r = rr.RRegex(p)
        lines = long_ascii_lines(rng, p, 200)
        want = dot_star(p, lines)
        check(r, b"\n".join(lines) + b"\n", want, stripes=(512, 1024, 4096, 0), what="long")
        # the same lines in a corpus that holds a high byte (in a line of its own): the other stride-2 kernel, the clamped wide table
        check(r, b"\n".join(lines) + b"\n\xc3\xa9", np.append(want, np.uint8(r.accepts_empty)), stripes=(1024, 0), what="long+high")


def test_every_table_form_gives_the_same_bitmap():
    rng = random.Random(882)
    for p in (EMAIL, "ab+c", "k(1|10|100)", U2, K1000_CONTAINS):
        regs = [rr.RRegex(p, e) for e in FORMS]
        names = [r.contains_engine_name for r in regs]
        assert names[1] in ("dfa-wide-table", "dfa-classed-table") and names[2] == "dfa-global-table", names
        if p != U2:
            assert names[0] == "dfa-stride2-table", names
        lines = long_ascii_lines(rng, p, 3000, maxlen=900)
        for i in range(0, len(lines), 7):                       # high bytes and NUL inside every seventh line
            ln = bytearray(lines[i])
            ln[rng.randrange(len(ln)):rng.randrange(len(ln))] = rng.choice([b"\xc3\xa9", b"\x00", b"\xff", b"\xe2\x82\xac"])
            lines[i] = bytes(ln)
        for ls in (lines, [ln for k, ln in enumerate(lines) if k % 7]):      # with and without high bytes in the corpus
            data = b"\n".join(ls) + b"\n"
            got = [contains(r, data, stripe) for r in regs for stripe in (1024, 0)]
            for g in got[1:]:
                assert (g == got[0]).all(), (p[:30], names, int(np.nonzero(g != got[0])[0][0]))
            sample = [k for k in range(0, len(ls), 9) if max(ls[k]) < 0x80 and min(ls[k]) > 0]
            assert (got[0][sample] == dot_star(p, [ls[k] for k in sample])).all(), p[:30]


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
def test_contains_equals_search_at_scale(kind):
    import synth
    pattern = {"url": U2, "email": EMAIL, "kwlog": K1000_CONTAINS}[kind]
    n = 256 << 20
    host = synth.corpus(kind, 6, n)
    r = rr.RRegex(pattern)
    for variant, text in (("as generated", host), ("utf-8 sprinkled", sprinkle_utf8(host, 3))):
        dev = torch.from_numpy(text).cuda()
        corpus = rr.Corpus(dev)
        bits = r.contains_corpus_bits(corpus)
        got = r.contains_corpus(corpus)
        s, e = r.search_corpus(corpus)
        found = (s != -1)
        assert torch.equal(got.bool(), found), (kind, variant, int(torch.nonzero(got.bool() != found)[0]))
        assert rr.bitmap_count(bits, corpus.num_lines) == int(found.sum()), (kind, variant)
        if variant == "as generated":
            starts = np.concatenate([[0], np.nonzero(host == 10)[0] + 1])
            got_host = got.cpu().numpy()
            for at in (0, 97 << 20, 201 << 20):                  # 1 MiB chunks against the oracle's .*(p).*
                first = int(np.searchsorted(starts, at))
                last = int(np.searchsorted(starts, at + (1 << 20)))
                lines = [host[starts[k]:starts[k + 1] - 1].tobytes() for k in range(first, min(last, len(starts) - 1))]
                assert (got_host[first:first + len(lines)] == dot_star(pattern, lines)).all(), (kind, at)
        del dev, corpus, bits, got, s, e, found


def test_line_geometry():
    """Lines longer than several stripes with the match at the start, across a stripe boundary, in the last two bytes, nowhere; at
    every alignment of the match to the byte pairs; a high byte as the last byte of a stripe and as the first behind it; 5-byte
    lines; corpus sizes that leave an odd tail byte.  Oracle: Python's re on a pattern whose semantics the dialects share."""
    p, needle = "ab+c", b"abbc"
    rx = re.compile(rb"ab+c")
    regs = [rr.RRegex(p, e) for e in FORMS]
    stripe = 1024
    for shift in range(0, 6):
        lines = []
        for length in (5000, 3 * stripe, 4097):
            fill = b"xy z" * (length // 4 + 1)
            lines += [needle + fill[:length], fill[:length], fill[:length - 4] + needle, fill[:length - 2] + b"ab",
                      fill[:length // 2] + needle + fill[:length // 2]]
        head = b"q" * shift + b"\n"
        data = head + b"\n".join(lines)
        # matches laid over every stripe boundary of the corpus, at offsets -3 ... +1 around it; high bytes on both sides of others
        a = bytearray(data)
        k = 0
        for b in range(stripe, len(a) - 8, stripe):
            if b"\n" in a[b - 6:b + 8]:
                continue
            if k % 2 == 0:
                off = b - 3 + (k // 2) % 5
                a[off:off + 4] = needle
            else:
                a[b - 1:b + 1] = b"\xc3\xa9"
                if k % 4 == 1:
                    a[b + 1:b + 5] = needle
            k += 1
        for tail in (b"", b"\n", b"a", b"ab", b"abbc", b"\xc3"):
            text = bytes(a) + tail
            want = np.array([1 if rx.search(ln) else 0 for ln in split_lines(text)], dtype=np.uint8)
            for r in regs:
                check(r, text, want, stripes=(stripe, 512), what="geometry shift %d tail %r" % (shift, tail))
    rng = random.Random(5)
    short = [bytes(rng.choice(b"abbc") for _ in range(4)) for _ in range(60000)]
    for text in (b"\n".join(short) + b"\n", b"\n".join(short), b"\n".join(short) + b"\n\xc3\xa9"):
        want = np.array([1 if rx.search(ln) else 0 for ln in split_lines(text)], dtype=np.uint8)
        for r in regs:
            check(r, text, want, stripes=(512, 0), what="5-byte lines")


def test_high_bytes_do_not_reject():
    text = b"caf\xc3\xa9 http://a.bc\nna\xc3\xafve\n\x00ftp://x.yz/z\nhttp://plain.org\nnothing here\n"
    want = np.array([1, 0, 1, 1, 0], dtype=np.uint8)
    for e in FORMS:
        check(rr.RRegex(U2, e), text, want)
    check(rr.RRegex(EMAIL), b"\xe2\x82\xac a@b\n\xff\xff\nx\x80@y\n\x80x@y\xff\n", np.array([1, 0, 0, 1], dtype=np.uint8))
    corpus = rr.Corpus(to_dev(text))
    whole = rr.RRegex(".*(" + U2 + ").*").match_corpus(corpus).cpu().numpy()
    assert list(whole) == [0, 0, 0, 1, 0]                        # the batch path rejects a line that holds such a byte


def test_bitmap_count():
    rng = np.random.default_rng(9)
    words = rng.integers(0, 1 << 32, size=(10**6 + 7 + 31) // 32 + 4, dtype=np.uint64).astype(np.uint32)
    words[-6:] = 0xffffffff                                      # the tail bits beyond every nlines below are set on purpose
    dev = torch.from_numpy(words.view(np.int32)).cuda()
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")
    for n in (0, 1, 31, 32, 33, 10**6 + 7):
        assert rr.bitmap_count(dev, n) == int(bits[:n].sum()), n
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    assert rr.bitmap_count(dev, 10**6 + 7, stream=st) == int(bits[:10**6 + 7].sum())


def test_streams_and_graph_replay():
    import synth
    r = rr.RRegex(EMAIL)
    hosts = [synth.corpus("email", 4, 8 << 20), sprinkle_utf8(synth.corpus("email", 5, 8 << 20), 1)]
    corpora = [rr.Corpus(torch.from_numpy(h).cuda()) for h in hosts]
    serial = [r.contains_corpus_bits(c).clone() for c in corpora]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [torch.empty_like(s) for s in serial]
    for _ in range(3):
        for c, st, o in zip(corpora, streams, outs):
            r.contains_corpus_bits(c, out=o, stream=st)
    torch.cuda.synchronize()
    assert all(torch.equal(o, s) for o, s in zip(outs, serial))
    # one branch, captured and replayed twice
    out = torch.zeros_like(serial[1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        r.contains_corpus_bits(corpora[1], out=out)              # (tables are up, nothing is allocated inside the capture)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            r.contains_corpus_bits(corpora[1], out=out)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        out.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, serial[1])


def test_degenerate_inputs():
    for e in FORMS:
        for p in ("ab?", "a*", "[]"):
            r = rr.RRegex(p, e)
            empty = rr.Corpus(torch.empty(0, dtype=torch.uint8, device="cuda"))
            assert r.contains_corpus_bits(empty).numel() == 0 and r.contains_corpus(empty).numel() == 0
            for data in (b"\n", b"\n\n\n", b"a", b"xab", b"abc\n", b"\xc3\xa9a"):
                want = np.zeros(len(split_lines(data)), dtype=np.uint8) if p == "[]" else brute_force(p, data)
                check(r, data, want)
    r, c = rr.RRegex("a"), rr.Corpus(to_dev(b"a\n"))
    assert rr._L.rrx_contains_corpus(None, c._h, None, None) == 2 and rr._L.rrx_contains_corpus(r._h, None, None, None) == 2
    assert rr._L.rrx_contains_corpus(r._h, c._h, None, None) == 2          # RRX_ERR_ARG: no bitmap for a corpus with lines
    assert rr._L.rrx_bitmap_count(0, None, 5, None, None) == 2
