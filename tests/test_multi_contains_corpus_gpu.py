"""rrx_multi_contains_corpus on the device: word i = the mask of line i of a '\\n'-corpus.  The references all come from code that
was there before the entry, run on the same device tensor:
  R1  RRegex(p).contains_corpus_bits(corpus) per distinct member (sets whose patterns hold no '\\n'),
  R2  RMulti.contains_extents over an offsets array built from the newline positions of the same bytes (trim 1; a text that does
      not end in '\\n' gets one appended in a copy),
  R3  on the short lines, multi_cases.want_masks: the CPU brute force.
Every case runs on three builds (builds(): one group if it fits, cut into groups by max_rows=8 so that the OR launches run, the
table in HBM/L2), through a poisoned buffer with guard words behind the last line."""
import os
import re

import numpy as np
import pytest

import roaringregex_amd as rr
from contains_cases import split_lines, unpack
from multi_cases import SETS, items_of, want_masks
from test_contains_items_lowering import oracle_for, shortest_accepted

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A        # no mask of SETS equals it: bit 30 is set (sets below 31 members), bit 12 without bit 0 ("thirtytwo": one pattern)
GUARD = 8                  # words behind nlines that no launch may touch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# lanes per workgroup, read from the source (device.hpp: RRX_THREADS, the default of kThreads)
THREADS = int(re.search(r"^#define RRX_THREADS (\d+)$", open(os.path.join(ROOT, "roaringregex_amd", "csrc", "device.hpp")).read(), re.M).group(1))
_regex, _builds, _large = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"


def member(p):
    if p not in _regex:
        _regex[p] = rr.RRegex(p)
    return _regex[p]


def builds(name):
    """(what, RMulti) of a set of SETS, compiled once per module: default, cut into three groups at least, global."""
    if name not in _builds:
        pats = SETS[name]
        cut = rr.RMulti(pats, max_rows=8)
        if len(pats) >= 5:
            assert cut.groups >= 3, cut.groups
        _builds[name] = [("default", rr.RMulti(pats)), ("cut", cut), ("global", rr.RMulti(pats, engine=rr.ENGINE_DFA_GLOBAL))]
    return _builds[name]


def as_array(data):
    return data if isinstance(data, np.ndarray) else np.frombuffer(bytes(data), dtype=np.uint8).copy()


def to_dev(a):
    return torch.from_numpy(a).cuda() if len(a) else torch.empty(0, dtype=torch.uint8, device="cuda")


def r1(pats, corpus):
    """uint32 per line from the single-pattern entry: bit k = bit i of RRegex(pats[k]).contains_corpus_bits, one call per distinct pattern."""
    n = corpus.num_lines
    cols, m = {}, np.zeros(n, dtype=np.uint32)
    for k, p in enumerate(pats):
        assert "\n" not in p
        if p not in cols:
            cols[p] = unpack(member(p).contains_corpus_bits(corpus).cpu().numpy(), n).astype(np.uint32) if n else np.zeros(0, np.uint32)
        m |= cols[p] << np.uint32(k)
    return m


def r2(m, corpus, host):
    """uint32 per line from the lane-per-item entry on the lines as items: offsets = the line starts, trim 1."""
    if not len(host):
        return np.zeros(0, dtype=np.uint32)
    dev = corpus.data
    if host[-1] != 10:
        host = np.append(host, np.uint8(10))
        dev = to_dev(host)
    offs = np.concatenate([[0], np.nonzero(host == 10)[0] + 1]).astype(np.int64)
    return m.contains_extents(dev, torch.from_numpy(offs).cuda(), trim=1).cpu().numpy().view(np.uint32)


def run(m, corpus, stream=None):
    """The masks as uint32 through a poisoned buffer with guard words behind nlines: every word written, none beyond."""
    n = corpus.num_lines
    buf = torch.full((n + GUARD,), POISON, dtype=torch.int32, device="cuda")
    out = m.contains_corpus(corpus, out=buf, stream=stream)
    torch.cuda.synchronize()
    assert out.numel() == n and out.data_ptr() == buf.data_ptr()
    assert (buf[n:] == POISON).all(), "words behind the masks were written"
    got = out.cpu().numpy().view(np.uint32)
    left = np.nonzero(got == np.uint32(POISON))[0]
    assert left.size == 0, ("words left unwritten", left[:8].tolist(), n)
    return got


def same(got, want, what, host=None):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (what, "line", int(bad[0]), hex(int(got[bad[0]])), hex(int(want[bad[0]])), None if host is None else split_lines(host)[bad[0]][:60])


def check(name, data, stripe=0, refs=("r1", "r2"), want=None, what=()):
    """One text on the three builds of a set against the references; -> (corpus, the masks)."""
    host = as_array(data)
    corpus = rr.Corpus(to_dev(host), stripe=stripe)
    assert corpus.num_lines == len(split_lines(host)), (name, what, corpus.num_lines)
    wants = []
    if want is not None:
        wants.append(("by hand", want))
    if "r1" in refs:
        wants.append(("R1", r1(SETS[name], corpus)))
    if "r2" in refs:
        wants.append(("R2", r2(builds(name)[0][1], corpus, host)))
    assert wants
    got = None
    for build, m in builds(name):
        got = run(m, corpus)
        for ref, w in wants:
            same(got, w, (name, what, "stripe", stripe, build, ref), host)
    return corpus, got


# ---- 1. short lines against the brute force
@pytest.mark.parametrize("name", [n for n in SETS if n != "newline"])
def test_short_lines_against_the_brute_force_and_the_members(name):
    items, want = items_of(name), want_masks(name)
    keep = [i for i, it in enumerate(items) if b"\n" not in it]
    assert len(keep) > len(items) // 2
    data = b"".join(items[i] + b"\n" for i in keep)
    check(name, data, want=want[keep], what="short lines")


def test_short_lines_of_the_set_with_newlines_in_its_patterns():
    """'\\n' inside the items replaced by 'z': a member whose pattern holds a '\\n' can match only through its '\\n'-free words."""
    lines = [it.replace(b"\n", b"z") for it in items_of("newline")]
    _, got = check("newline", b"".join(ln + b"\n" for ln in lines), refs=("r2",), what="short lines")
    assert not (got & np.uint32(0b000110)).any()                    # "a\nb" and "k\n+1" have no such word
    assert (got & np.uint32(0b001000)).any() and (got & np.uint32(1)).any()


# ---- 2. stripe geometry at the smallest stripe
def geometry_corpus():
    """-> (bytes, {line: expected word}) for the set "nullable": bit 0 a* (every line), 1 ab+c, 2 (a|b)*abb, 3 [0-9]+\\.[0-9]+, 4 e-mail."""
    buf, want = bytearray(), {}

    def fill_to(pos, plant=()):
        """'z' up to byte `pos` (exclusive) of the text, with `plant` = (absolute offset, bytes) laid over it."""
        at = len(buf)
        assert pos >= at
        buf.extend(b"z" * (pos - at))
        for off, word in plant:
            assert at <= off and off + len(word) <= pos
            buf[off:off + len(word)] = word

    def end_line(word):
        want[bytes(buf).count(b"\n")] = word
        buf.extend(b"\n")

    fill_to(511, [(0, b"abbc")]); end_line(0b00111)                  # line 0 ends exactly on the last byte of stripe 0
    fill_to(1024, [(600, b"1.5")]); end_line(0b01001)                # line 1: all of stripe 1; its '\n' is the first byte of stripe 2
    start = len(buf)                                                 # line 2: 1300 bytes, stripe 3 (1536 .. 2047) holds no '\n'
    fill_to(start + 1300, [(1700, b"a@b"), (2100, b"abc")]); end_line(0b10011)
    assert start < 1536 and len(buf) > 2048
    fill_to(2559); end_line(0b00001); end_line(0b00001)              # "\n\n" astride 2559 | 2560: an empty line
    fill_to(3070); end_line(0b00001); end_line(0b00001); end_line(0b00001)       # "\n\n\n" at 3070, 3071 | 3072: two empty lines
    # "abc" across the stripe boundary 3583 | 3584, "1.5" across the 16-byte boundary 3631 | 3632
    fill_to(3700, [(3582, b"abc"), (3630, b"1.5")]); end_line(0b01011)
    buf.extend(b"zzab"); end_line(0b00001)                           # "ab" '\n' "c": no match spans the '\n'
    buf.extend(b"czz"); end_line(0b00001)
    # every bit within the first 8 bytes, then 700 bytes that hold the neighbours of '\n' but no '\n': the early exit must find the right one
    buf.extend(b"abbc@1.5" + b"z\x0b\x09\x8a" * 175); end_line(0b11111)
    buf.extend(b"zz1.5zz"); end_line(0b01001)
    buf.extend(b"zabbz"); end_line(0b00101)
    buf.extend(b"a@b"); end_line(0b10001)
    return bytes(buf), want


@pytest.mark.parametrize("stripe", [512, 1024, 16384])
def test_stripe_geometry(stripe):
    data, planted = geometry_corpus()
    assert data[511] == 10 and data[1024] == 10 and b"\n" not in data[1536:2048] and data[2559:2561] == b"\n\n" and data[3070:3073] == b"\n\n\n"
    assert data[3582:3585] == b"abc" and data[3630:3633] == b"1.5"
    corpus, got = check("nullable", data, stripe=stripe, what="geometry")
    assert corpus.stripe == stripe and corpus.num_lines == len(planted) == 15
    same(got, np.array([planted[i] for i in range(15)], dtype=np.uint32), ("geometry by hand", stripe), as_array(data))


# ---- 3. ends of the data
def random_text(rng, n):
    alphabet = np.frombuffer(b"abc1.@z5abz\n", dtype=np.uint8)          # one byte in twelve a '\\n'
    return alphabet[rng.integers(0, len(alphabet), size=n)]


@pytest.mark.parametrize("n", [1, 15, 16, 17, 511, 512, 513, 4097])
def test_lengths_around_a_load_and_a_stripe(n):
    rng = np.random.default_rng(4400 + n)
    text = random_text(rng, n)
    for last in (10, ord("c")):                                      # with and without a final '\n'
        text[-1] = last
        check("nullable", text.copy(), stripe=512, what=("length", n, "last byte", last))


def test_a_final_newline_or_none_one_line_and_only_newlines():
    short = b"abbc\nzz1.5\n\na@b zabc\nabb"
    c1, with_nl = check("nullable", short + b"\n", stripe=512, what="final newline")
    c2, without = check("nullable", short, stripe=512, what="no final newline")
    assert c1.num_lines == c2.num_lines == 5 and (with_nl == without).all() and with_nl.tolist() == [0b00111, 0b01001, 0b00001, 0b10011, 0b00101]
    one = bytearray(b"z" * 700)
    one[510:513], one[690:693] = b"abc", b"a@b"
    corpus, got = check("nullable", bytes(one), stripe=512, what="one line")
    assert corpus.num_lines == 1 and got.tolist() == [0b10011]
    corpus, got = check("nullable", b"\n" * 600, stripe=512, what="only newlines")
    assert corpus.num_lines == 600 and (got == 1).all()              # the nullable member's bit, 600 times


# ---- 4. stripe counts around the wave and the workgroup
@pytest.mark.parametrize("nstripes", [1, 63, 64, 65, THREADS - 1, THREADS, THREADS + 1])
def test_stripe_counts_around_the_wave_and_the_workgroup(nstripes):
    assert THREADS in (256, 512, 1024)
    base = [it for it in items_of("twelve") if b"\n" not in it]
    nbytes = (nstripes - 1) * 512 + 100
    buf, i = bytearray(), 0
    while len(buf) < nbytes:
        buf += base[(7 * i) % len(base)] + b"\n"
        i += 1
    corpus, got = check("twelve", bytes(buf[:nbytes]), stripe=512, refs=("r1",), what=("stripes", nstripes))
    assert (corpus.num_bytes + 511) // 512 == nstripes and (nstripes < 63 or len(set(got.tolist())) > 4)


# ---- 5. a large random corpus
def large_text(pats, seed, nbytes=4 << 20):
    """About 4 MiB over large_batch's alphabet: lines of 0 .. 120 bytes, every 2000th one of 2 .. 5 KiB, a member's shortest
    '\\n'-free accepted word planted in one line in three."""
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"abcxk01.d@yz:/hftps \x00\xff", dtype=np.uint8)
    text = alphabet[rng.integers(0, len(alphabet), size=nbytes)]
    lens = rng.integers(0, 121, size=nbytes // 50)
    lens[::2000] = rng.integers(2048, 5121, size=len(lens[::2000]))
    ends = np.cumsum(lens + 1) - 1                                   # the '\n' of line i
    ends = ends[ends < nbytes]
    text[ends] = 10
    starts = np.concatenate([[0], ends[:-1] + 1])
    needles = []
    for p in dict.fromkeys(pats):
        w = shortest_accepted(oracle_for(p))
        if w and "\n" not in p:
            needles.append(np.frombuffer(w, dtype=np.uint8))
    for i in range(0, len(ends), 3):
        nd = needles[(i // 3) % len(needles)]
        b, e = int(starts[i]), int(ends[i])
        if e - b >= len(nd):
            at = b + int(rng.integers(0, e - b - len(nd) + 1))
            text[at:at + len(nd)] = nd
    return text[:int(ends[-1]) + 1 - (seed & 1)].copy()              # (an odd seed: the last line without its '\n')


def large(name):
    """(corpus, the masks of the default build, checked on all three builds) of a set, once per module."""
    if name not in _large:
        pats = SETS[name]
        text = large_text(pats, 4500 + len(name))
        assert len(text) > 3 << 20
        refs = {"newline": ("r2",), "twelve": ("r1", "r2")}.get(name, ("r1",))
        corpus, got = check(name, text, refs=refs, what="large")
        lines = split_lines(text[:1 << 16])
        assert corpus.num_lines > 50_000 and min(map(len, lines)) == 0 and max(map(len, lines)) > 2048
        if "r1" in refs:
            for k, p in enumerate(pats):                             # every member that can show both verdicts does
                col = int(((got >> np.uint32(k)) & 1).sum())
                assert (col == len(got)) if member(p).accepts_empty else (0 < col < len(got)), (name, k, col)
        _large[name] = (corpus, got)
    return _large[name]


@pytest.mark.parametrize("name", list(SETS))
def test_a_large_corpus_against_the_members(name):
    large(name)


# ---- 6. the readers of a mask column
def test_counts_and_planes_of_the_large_corpus():
    pats = SETS["thirtytwo"]
    corpus, host = large("thirtytwo")
    m = builds("thirtytwo")[0][1]
    masks = m.contains_corpus(corpus)
    n = corpus.num_lines
    assert (masks.cpu().numpy().view(np.uint32) == host).all()
    counts = m.counts(masks).cpu().numpy()
    assert counts.tolist() == [int(((host >> np.uint32(k)) & 1).sum()) for k in range(32)]
    nw = (n + 31) // 32
    for k in (0, 11, 31):
        out = torch.full((nw + GUARD,), POISON, dtype=torch.int32, device="cuda")
        plane = m.plane(masks, k, out=out)
        assert torch.equal(plane, member(pats[k]).contains_corpus_bits(corpus)), k                  # word for word
        assert (out[nw:] == POISON).all() and rr.bitmap_count(plane, n) == int(counts[k])


# ---- 7. empty languages and empty input
def test_empty_languages_cost_a_memset_and_an_empty_corpus_nothing():
    host = as_array(b"".join(ln + b"\n" for ln in items_of("one")[:100] if b"\n" not in ln))
    corpus = rr.Corpus(to_dev(host), stripe=512)
    n = corpus.num_lines
    same(run(rr.RMulti(["[]", "[]"]), corpus), np.zeros(n, dtype=np.uint32), "the empty languages")
    first_empty = rr.RMulti(["[]", "ab+c"], max_rows=1)
    assert first_empty.groups == 2
    want = r1(["ab+c"], corpus) << np.uint32(1)
    assert want.any()
    same(run(first_empty, corpus), want, "an empty first group")
    # rrx_corpus_create admits a zero-byte corpus: no line, no word
    empty = rr.Corpus(torch.empty(0, dtype=torch.uint8, device="cuda"))
    assert empty.num_lines == 0
    buf = torch.full((GUARD,), POISON, dtype=torch.int32, device="cuda")
    one = rr.RMulti(["a"])
    assert one.contains_corpus(empty, out=buf).numel() == 0
    nullable = rr.RMulti(["a*"])
    assert rr._L.rrx_multi_contains_corpus(nullable._h, empty._h, buf.data_ptr(), None) == 0        # the entry itself, a*: still no word
    torch.cuda.synchronize()
    assert (buf == POISON).all()


# ---- 8. a side stream and a captured graph
def test_a_side_stream_and_a_captured_graph():
    data, _ = geometry_corpus()
    corpus = rr.Corpus(to_dev(as_array(data)), stripe=512)
    n = corpus.num_lines
    m = builds("nullable")[1][1]
    assert m.groups >= 3
    eager = m.contains_corpus(corpus).clone()
    same(eager.cpu().numpy().view(np.uint32), r1(SETS["nullable"], corpus), "eager")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    out = torch.full((n + GUARD,), POISON, dtype=torch.int32, device="cuda")
    got = m.contains_corpus(corpus, out=out, stream=side)
    side.synchronize()
    assert torch.equal(got, eager) and (out[n:] == POISON).all()
    out.fill_(0)
    with torch.cuda.stream(side):
        m.contains_corpus(corpus, out=out)                             # (tables are up, nothing is allocated inside the capture)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            m.contains_corpus(corpus, out=out)
    torch.cuda.current_stream().wait_stream(side)
    out.fill_(POISON)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[:n], eager) and (out[n:] == POISON).all()
