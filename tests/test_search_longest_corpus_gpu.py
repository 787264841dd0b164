"""rrx_search_longest_corpus on the device: words i = the leftmost-longest match of line i of a '\\n'-corpus.  The references come
from code that was there before the entry:
  R1  RRegex.search_longest_extents over an offsets array built from the newline positions of the same bytes (trim 1; a text that
      does not end in '\\n' gets one appended in a copy),
  R2  on short lines the CPU brute force (test_search_longest_items_lowering.want_for), and the rows of
      search_longest_corpus_cases.geometry_wants for the corpus built by hand.
Every case runs on the default build and with the tables forced into HBM/L2 (builds()), GLOBAL_AUTO - global by size - on the
geometry and the short lines, through buffers poisoned with 0x5A5A5A5A and guard words behind the last line."""
import os
import random
import re

import numpy as np
import pytest

import roaringregex_amd as rr
from contains_cases import EXPLODING, split_lines
from patterns import EMAIL, K1000_CONTAINS, U2
from search_longest_corpus_cases import GEOMETRY_PATTERNS, geometry_corpus, geometry_wants, reference_texts
from table_edge_cases import plain_table_bytes
from test_search_longest_items_lowering import GLOBAL_AUTO, global_auto_items, want_for

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A        # no offset of these texts: the largest is 4 MiB
GUARD = 8                  # words behind the lines that no launch may touch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# lanes per workgroup, read from the source (device.hpp: RRX_THREADS, the default of kThreads)
THREADS = int(re.search(r"^#define RRX_THREADS (\d+)$", open(os.path.join(ROOT, "roaringregex_amd", "csrc", "device.hpp")).read(), re.M).group(1))
_builds, _large = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"


def builds(p):
    """(what, RRegex) of a pattern, compiled once per module: the default placement and both tables in HBM/L2."""
    if p not in _builds:
        _builds[p] = [("default", rr.RRegex(p)), ("global", rr.RRegex(p, rr.ENGINE_DFA_GLOBAL))]
    return _builds[p]


def as_array(data):
    return data if isinstance(data, np.ndarray) else np.frombuffer(bytes(data), dtype=np.uint8).copy()


def to_dev(a):
    return torch.from_numpy(a).cuda() if len(a) else torch.empty(0, dtype=torch.uint8, device="cuda")


def r1(r, corpus, host):
    """int32 [lines, 2] from the lane-per-item entry on the lines as items: offsets = the line starts, trim 1."""
    if not len(host):
        return np.zeros((0, 2), dtype=np.int32)
    dev = corpus.data
    if host[-1] != 10:
        host = np.append(host, np.uint8(10))
        dev = to_dev(host)
    offs = np.concatenate([[0], np.nonzero(host == 10)[0] + 1]).astype(np.int64)
    s, e = r.search_longest_extents(dev, torch.from_numpy(offs).cuda(), trim=1)
    return torch.stack([s, e], dim=1).cpu().numpy()


def run(r, corpus, expect_rc=0, stream=None, bufs=None):
    """The entry itself on poisoned buffers with guard words behind the lines -> int32 [lines, 2]: every word written, none beyond
    (a refused call: none at all)."""
    n = corpus.num_lines
    st, en = bufs or (torch.empty(n + GUARD, dtype=torch.int32, device="cuda"), torch.empty(n + GUARD, dtype=torch.int32, device="cuda"))
    st.fill_(POISON)
    en.fill_(POISON)
    torch.cuda.synchronize()                                         # (the fills ran on the current stream)
    rc = rr._L.rrx_search_longest_corpus(r._h, corpus._h, st.data_ptr(), en.data_ptr(), rr._stream_ptr(stream))
    assert rc == expect_rc, (rc, rr._L.rrx_last_error())
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    assert (st[n:] == POISON).all() and (en[n:] == POISON).all(), "words behind the lines were written"
    got = torch.stack([st[:n], en[:n]], dim=1).cpu().numpy()
    if expect_rc:
        assert (got == POISON).all(), "a refused call wrote a result word"
    else:
        left = np.nonzero((got == POISON).any(axis=1))[0]
        assert left.size == 0, ("words left unwritten", left[:8].tolist(), n)
    return got


def same(got, want, what, host=None):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (what, "line", int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist(), None if host is None else split_lines(host)[bad[0]][:60])


def check(p, data, stripe=0, want=None, what=(), regexes=None):
    """One text on every build of a pattern against R1 (and `want`); -> (corpus, the rows)."""
    host = as_array(data)
    corpus = rr.Corpus(to_dev(host), stripe=stripe)
    assert corpus.num_lines == len(split_lines(host)), (p, what, corpus.num_lines)
    regexes = regexes or builds(p)
    wants = [("R1", r1(regexes[0][1], corpus, host))] + ([("by hand", want)] if want is not None else [])
    got = None
    for build, r in regexes:
        got = run(r, corpus)
        for ref, w in wants:
            same(got, w, (p[:30], what, "stripe", stripe, build, ref), host)
    return corpus, got


# ---- 1. short lines against the brute force
def test_short_lines_against_the_brute_force():
    for p, text, want in reference_texts():
        for stripe in (512, 1024):
            check(p, text, stripe=stripe, want=want, what="short lines")
    r = rr.RRegex(GLOBAL_AUTO)
    assert plain_table_bytes(r.program(rr.PROGRAM_SEARCH_STARTS)) + plain_table_bytes(r.program(rr.PROGRAM_SEARCH_ANCHORED)) > 65536
    items = global_auto_items(random.Random(32), 300)
    want = want_for(GLOBAL_AUTO, items)
    assert 5 < int((want[:, 1] >= 0).sum()) < len(items)
    check(GLOBAL_AUTO, b"".join(it + b"\n" for it in items), stripe=512, want=want, what="global by size", regexes=[("auto", r)])


# ---- 2. stripe geometry
@pytest.mark.parametrize("stripe", [512, 1024, 16384])
def test_stripe_geometry(stripe):
    data, _, _ = geometry_corpus()
    wants = geometry_wants()
    for p in GEOMETRY_PATTERNS:
        corpus, _ = check(p, data, stripe=stripe, want=wants[p], what="geometry")
        assert corpus.stripe == stripe
    check(GLOBAL_AUTO, data, stripe=stripe, what="geometry, global by size", regexes=[("auto", rr.RRegex(GLOBAL_AUTO))])


# ---- 3. ends of the data
EDGE_PATTERNS = ["ab+c", "(a|b)*abb", "[0-9]+\\.[0-9]+|\\.", "a*"]


def random_text(rng, n):
    alphabet = np.frombuffer(b"abc1.@z5abz\n", dtype=np.uint8)          # one byte in twelve a '\\n'
    return alphabet[rng.integers(0, len(alphabet), size=n)]


@pytest.mark.parametrize("n", [1, 15, 16, 17, 511, 512, 513, 4097])
def test_lengths_around_a_load_and_a_stripe(n):
    rng = np.random.default_rng(5400 + n)
    text = random_text(rng, n)
    for last in (10, ord("c")):                                      # with and without a final '\n'
        text[-1] = last
        for p in EDGE_PATTERNS:
            check(p, text.copy(), stripe=512, what=("length", n, "last byte", last))


def test_a_final_newline_or_none_one_line_only_newlines_and_a_shared_last_stripe():
    short = b"abbc\nzz1.5\n\na@b zabc\nabb"
    c1, with_nl = check("ab+c", short + b"\n", stripe=512, what="final newline")
    c2, without = check("ab+c", short, stripe=512, what="no final newline")
    assert c1.num_lines == c2.num_lines == 5 and (with_nl == without).all() and with_nl.tolist() == [[0, 4], [-1, -1], [-1, -1], [5, 8], [-1, -1]]
    one = bytearray(b"z" * 700)
    one[510:513], one[690:694] = b"abc", b"abbc"
    corpus, got = check("ab+c", bytes(one), stripe=512, what="one line")
    assert corpus.num_lines == 1 and got.tolist() == [[510, 513]]
    for p, row in (("ab+c", [-1, -1]), ("a*", [0, 0])):
        corpus, got = check(p, b"\n" * 600, stripe=512, what="only newlines")
        assert corpus.num_lines == 600 and (got == row).all()
    # the last stripe ends two lines and holds the final fragment, whose match begins in the stripe before
    tail = bytearray(b"z" * 1100)
    tail[400], tail[1030], tail[1060] = 10, 10, 10
    tail[1020:1026], tail[1090:1094] = b"abbbbc", b"abbc"
    corpus, got = check("ab+c", bytes(tail), stripe=512, what="a fragment in a shared last stripe")
    assert got.tolist() == [[-1, -1], [1020 - 401, 1026 - 401], [-1, -1], [1090 - 1061, 1094 - 1061]]
    for p in EDGE_PATTERNS:
        check(p, bytes(tail), stripe=512, what="a fragment in a shared last stripe")


# ---- 4. stripe counts around the wave and the workgroup
@pytest.mark.parametrize("nstripes", [1, 63, 64, 65, THREADS - 1, THREADS, THREADS + 1])
def test_stripe_counts_around_the_wave_and_the_workgroup(nstripes):
    assert THREADS in (256, 512, 1024)
    p, text, _ = next(t for t in reference_texts() if t[0] == EMAIL)
    base = split_lines(text)
    nbytes = (nstripes - 1) * 512 + 100
    buf, i = bytearray(), 0
    while len(buf) < nbytes:
        buf += base[(7 * i) % len(base)] + b"\n"
        i += 1
    corpus, got = check(p, bytes(buf[:nbytes]), stripe=512, what=("stripes", nstripes))
    assert (corpus.num_bytes + 511) // 512 == nstripes and (nstripes < 63 or 0 < int((got[:, 0] >= 0).sum()) < len(got))


# ---- 5. nullable, the empty language, tables that do not determinise, no line at all
def test_edge_patterns_and_output_buffers():
    data, _, _ = geometry_corpus()
    host = as_array(data)
    corpus = rr.Corpus(to_dev(host), stripe=512)
    lines = split_lines(data)
    for build, r in builds("a*"):                                    # every line [0, k), the empty ones [0, 0)
        got = run(r, corpus)
        same(got, np.array([(0, len(ln) - len(ln.lstrip(b"a"))) for ln in lines], dtype=np.int32), ("nullable", build), host)
        assert (got[[4, 6, 7]] == 0).all() and not lines[4] and got[:, 1].max() == 1
    for engine in (rr.ENGINE_AUTO, rr.ENGINE_DFA_GLOBAL):
        assert (run(rr.RRegex("[]", engine), corpus) == -1).all()    # the empty language: two fills
    run(rr.RRegex(EXPLODING), corpus, expect_rc=4)                   # RRX_ERR_UNSUPPORTED: the buffers stay as they were
    assert b"determinise" in rr._L.rrx_last_error()
    with pytest.raises(rr.RRegexError, match="determinise"):
        rr.RRegex(EXPLODING).search_longest_corpus(corpus)
    s, e = rr.RRegex("ab+c").search_longest_corpus(corpus)           # the Python layer
    same(torch.stack([s, e], dim=1).cpu().numpy(), geometry_wants()["ab+c"], "RRegex.search_longest_corpus", host)
    # rrx_corpus_create admits a zero-byte corpus: no line, no word - and a regex without tables is still reported
    empty = rr.Corpus(torch.empty(0, dtype=torch.uint8, device="cuda"))
    assert empty.num_lines == 0
    for p in ("ab+c", "a*", "[]"):
        assert run(rr.RRegex(p), empty).shape == (0, 2)
        s, e = rr.RRegex(p).search_longest_corpus(empty)
        assert s.numel() == 0 and e.numel() == 0
    run(rr.RRegex(EXPLODING), empty, expect_rc=4)


# ---- 6. 4 MiB per config
def large_text(kind, seed, nbytes=4 << 20):
    """The synthetic corpus of a config cut into lines of our own: 0 .. 120 bytes, every 2000th one 2 .. 5 KiB."""
    import synth
    text = synth.corpus(kind, seed, nbytes).copy()
    text[text == 10] = ord(" ")
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 121, size=nbytes // 50)
    lens[::2000] = rng.integers(2048, 5121, size=len(lens[::2000]))
    ends = np.cumsum(lens + 1) - 1                                   # the '\n' of line i
    ends = ends[ends < nbytes]
    text[ends] = 10
    return text[:int(ends[-1]) + 1 - (seed & 1)].copy()              # (an odd seed: the last line without its '\n')


@pytest.mark.parametrize("kind", ["url", "email", "kwlog"])
def test_a_large_corpus_against_the_items_entry_and_the_first_match(kind):
    p = {"url": U2, "email": EMAIL, "kwlog": K1000_CONTAINS}[kind]
    text = large_text(kind, {"url": 6, "email": 7, "kwlog": 8}[kind])
    assert len(text) > 3 << 20
    corpus, got = check(p, text, what=("large", kind))
    lines = split_lines(text[:1 << 17])
    assert corpus.num_lines > 50_000 and min(map(len, lines)) == 0 and max(map(len, lines)) > 2048
    found = got[:, 0] >= 0
    assert 0 < int(found.sum()) and (kind == "kwlog" or int(found.sum()) < len(got))
    assert (got[found, 0] < got[found, 1]).all() and ((got[:, 1] >= 0) == found).all()
    # the other question on the same lines: found on the same ones, its match no further left and ending no later
    r = builds(p)[0][1]
    try:
        ss, se = r.search_corpus(corpus)
    except rr.RRegexError:                                           # (a pattern that rrx_search_corpus does not take: nothing to compare)
        return
    ss, se = ss.cpu().numpy(), se.cpu().numpy()
    assert ((se >= 0) == found).all(), (kind, "found-ness")
    assert (got[found, 0] <= ss[found]).all() and (got[found, 1] >= se[found]).all(), kind


# ---- 7. a side stream and a captured graph
def test_a_side_stream_and_a_captured_graph():
    data, _, _ = geometry_corpus()
    host = as_array(data)
    corpus = rr.Corpus(to_dev(host), stripe=512)
    n = corpus.num_lines
    for p in ("ab+c", "a*"):
        r, want = builds(p)[0][1], geometry_wants()[p]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        same(run(r, corpus, stream=side), want, (p, "side stream"), host)       # (eager: the tables are uploaded here)
        st = torch.full((n + GUARD,), POISON, dtype=torch.int32, device="cuda")
        en = torch.full((n + GUARD,), POISON, dtype=torch.int32, device="cuda")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                rr._check(rr._L.rrx_search_longest_corpus(r._h, corpus._h, st.data_ptr(), en.data_ptr(), rr._stream_ptr(side)))
        torch.cuda.current_stream().wait_stream(side)
        for round_ in range(2):
            st.fill_(POISON)
            en.fill_(POISON)
            g.replay()
            torch.cuda.synchronize()
            same(torch.stack([st[:n], en[:n]], dim=1).cpu().numpy(), want, (p, "replay", round_), host)
            assert (st[n:] == POISON).all() and (en[n:] == POISON).all()
