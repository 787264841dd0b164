"""The stride-2 match kernels on the byte-wide pair table (csrc/device.hpp: Dfa2Device::P8) against the oracle, line by line, on
corpora of 64 KiB - 1 MiB with 512-byte stripes (a workgroup's text: 512 KiB).  A table takes the byte-wide form exactly when
(ncols - 1) * 4 << rep_log2 <= 255: U2 (46 columns, one copy), (ab|cd|ef|gh){3,20}z (30 columns, two copies) and a{1,300} (7 columns,
two copies; the oracle takes a second per 25 KiB of it: small corpora only) do, the email regex (32 copies) and (a|b)*abb(a|b)*
stay on the u16 table - all of them run here, so a difference between the two builds shows as a difference to
the oracle on one side only.  Every call writes into a DIRTY bitmap: a word the kernel does not store shows at once.
Covered: both flush instantiations (period compiled in / per launch; mean line length above and below 33 bytes), both write-outs
(own words / cleared bitmap: a line longer than a workgroup's text), the kernel for text with bytes >= 0x80 (through contains),
and the edges of the pair step: 0x00 and 0x7f on either byte of a pair, '\\n' on either byte, an odd corpus length, a last line
without '\\n', lines across a stripe end and across a workgroup end, a corpus shorter than one 128-byte round."""
import numpy as np
import pytest

import roaringregex_amd as rr
from contains_cases import dot_star, split_lines
from patterns import EMAIL, U2
from pyoracle import OracleRegex

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

A300 = "a{1,300}"
PAIRS = "(ab|cd|ef|gh){3,20}z"                         # 103 rows of 30 columns, two interleaved copies: offsets up to 232
ABB = "(a|b)*abb(a|b)*"
HOSTS = r"(http|ftp)://[a-z]{1,30}\.[a-z]{2,3}"      # its CONTAINS table: 159 rows of 25 columns, one copy - byte-wide
WG_BYTES = 1024 * 512                                # a workgroup's text at stripe 512
FILLS = (-1, 0x55555555, -0x21524111, 0x7FFFFFFF)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"


def byte_wide(words):
    """The host's rule (pack.cpp: dfa2_copies_log2, dfa2_byte_pairs_fit) on a stride-2 program's header words."""
    D, C = int(words[0]), int(words[1])
    rep = 0
    while rep < 5 and D * (C | 1) * 4 * (2 << rep) <= 30 * 1024 and C * 4 * (2 << rep) <= 65535:
        rep += 1
    return ((C - 1) * 4 << rep) <= 255


def regex(p):
    r = rr.RRegex(p)
    r.set_background_order(False)
    assert r.engine_name == "dfa-stride2-table"
    return r


def words_of(want, nwords):
    bits = np.zeros(nwords * 32, dtype=np.uint8)
    bits[:len(want)] = want
    return np.packbits(bits, bitorder="little").view(np.uint32)


def run_dirty(call, corpus, want, fill=-1, what=""):
    """call(corpus, out=) over a bitmap pre-filled with `fill`, eight words longer than needed: every word equals the oracle's,
    the words behind the bitmap are untouched."""
    nw = (corpus.num_lines + 31) // 32
    assert len(want) == corpus.num_lines, (what, len(want), corpus.num_lines)
    out = torch.full((nw + 8,), fill, dtype=torch.int32, device="cuda")
    got = call(corpus, out=out)
    torch.cuda.synchronize()
    assert got.numel() == nw
    host = out.cpu().numpy().view(np.uint32)
    ref = words_of(want, nw)
    bad = np.nonzero(host[:nw] != ref)[0]
    assert bad.size == 0, (what, "word", int(bad[0]), "of", nw, hex(int(host[bad[0]])), hex(int(ref[bad[0]])))
    assert (host[nw:] == np.uint32(fill & 0xFFFFFFFF)).all(), (what, "words behind the bitmap were written")


def both_flush_forms(p, call_of, corpus, want, what):
    """The automatic period, then the period compiled in (32 slots) and one taken per launch (4 slots)."""
    for k, slots in enumerate((0, 32, 4)):
        r = regex(p)
        r.set_flush_slots(slots)
        if slots:
            assert r.flush_slots(corpus) == (slots, slots == 32)
        run_dirty(call_of(r), corpus, want, fill=FILLS[k], what=(what, "flush slots", slots))


def test_which_tables_are_byte_wide():
    assert byte_wide(rr.RRegex(U2).program(rr.ENGINE_DFA2)) and byte_wide(rr.RRegex(A300).program(rr.ENGINE_DFA2))
    assert byte_wide(rr.RRegex(PAIRS).program(rr.ENGINE_DFA2))
    assert not byte_wide(rr.RRegex(EMAIL).program(rr.ENGINE_DFA2)) and not byte_wide(rr.RRegex(ABB).program(rr.ENGINE_DFA2))
    assert byte_wide(rr.RRegex(HOSTS).program(rr.PROGRAM_CONTAINS_DFA2)) and rr.RRegex(HOSTS).contains_engine_name == "dfa-stride2-table"


def pair_lines(seed, nbytes):
    """Text for PAIRS: 1 ... 40 of its pairs and a z per line (42 bytes on average), a byte replaced in three lines of ten, the first dropped in a few."""
    rng = np.random.default_rng(seed)
    pairs = [b"ab", b"cd", b"ef", b"gh"]
    out, size = [], 0
    while size < nbytes:
        ln = bytearray(b"".join(pairs[i] for i in rng.integers(0, 4, size=int(rng.integers(1, 41)))) + b"z")
        if rng.random() < 0.3:
            ln[int(rng.integers(len(ln)))] = b"abzq"[int(rng.integers(4))]
        elif rng.random() < 0.1:
            del ln[0]                                                # (lines are of odd length otherwise: '\n' on one parity only)
        out.append(bytes(ln))
        size += len(ln) + 1
    return np.frombuffer(b"\n".join(out) + b"\n", dtype=np.uint8)[:nbytes].copy()


def synthetic(kind, seed, nbytes):
    import synth
    return pair_lines(seed, nbytes) if kind == "pairs" else synth.corpus(kind, seed, nbytes)


def ab_lines(rng, nbytes, mean):
    a = np.frombuffer(b"ab\n", dtype=np.uint8)
    q = 1.0 / mean
    return a[rng.choice(3, size=nbytes, p=[(1 - q) / 2, (1 - q) / 2, q])].copy()


@pytest.mark.parametrize("p,kind", [(U2, "url"), (PAIRS, "pairs"), (EMAIL, "email"), (ABB, "ab")])
def test_two_workgroups_against_the_oracle(p, kind):
    """640 KiB + 77 bytes (odd, the last line cut short: no '\\n'): two workgroups that share a bitmap word, lines across every
    stripe end and across the workgroup end; the three flush settings each."""
    n = 640 * 1024 + 77
    data = ab_lines(np.random.default_rng(3), n, 48) if kind == "ab" else synthetic(kind, 11, n + 1)[:n].copy()
    for at in (WG_BYTES - 1, WG_BYTES, n - 1):                       # a line across the workgroup end, a last line without '\n'
        if data[at] == 10:
            data[at] = ord("a")
    assert len(data) % 2 == 1 and data[WG_BYTES - 1] != 10 and data[WG_BYTES] != 10 and (data[511::512] != 10).any()
    nl = np.nonzero(data == 10)[0]
    assert (nl % 2 == 0).any() and (nl % 2 == 1).any()               # '\n' on the even and on the odd byte of a pair
    want = OracleRegex(p).match_lines(data)
    assert 0 < int(want.sum()) < len(want)
    corpus = rr.Corpus(torch.from_numpy(data).cuda(), stripe=512)
    assert corpus.stripe == 512 and corpus.one_launch
    mean = len(data) / len(want)                                     # (email text: 24 bytes per line - the per-launch form)
    assert not 28 < mean < 36 and regex(p).flush_slots(corpus)[1] == (mean > 32), (kind, mean)
    both_flush_forms(p, lambda r: r.match_corpus_bits, corpus, want, kind)


def short_url_lines(rng, nbytes):
    """URL text of fewer than 33 bytes per line: short valid URLs among prefixes of longer ones."""
    valid = [b"ftp://a.bc", b"http://x-y.io/z", b"https://ab.cde:80/", b"http://q.w.er/t?y#u", b"ftp://abcdefghijklmnop.qr"]
    long_lines = split_lines(synthetic("url", 12, 256 * 1024).tobytes())
    out, size = [], 0
    while size < nbytes:
        ln = valid[rng.integers(len(valid))] if rng.random() < 0.4 else long_lines[rng.integers(len(long_lines))][:rng.integers(0, 30)]
        out.append(ln)
        size += len(ln) + 1
    return np.frombuffer(b"\n".join(out) + b"\n", dtype=np.uint8).copy()


def test_short_lines_take_the_per_launch_flush_form():
    """U2 on lines of about 15 bytes, 200 KiB: the automatic period is below 32 slots, the kernel that takes it per launch."""
    data = short_url_lines(np.random.default_rng(5), 200 * 1024)
    want = OracleRegex(U2).match_lines(data)
    assert len(data) / len(want) < 33 and 0 < int(want.sum()) < len(want)
    corpus = rr.Corpus(torch.from_numpy(data).cuda(), stripe=512)
    r = regex(U2)
    period, compiled_in = r.flush_slots(corpus)
    assert period < 32 and not compiled_in and corpus.one_launch
    run_dirty(r.match_corpus_bits, corpus, want, what="short url lines")


@pytest.mark.parametrize("p,kind,filler", [(U2, "url", b"hftp:/.-az09?#"), (PAIRS, "pairs", b"abcdefgh")])
def test_a_line_longer_than_a_workgroup_takes_the_clearing_path(p, kind, filler):
    """A line of 600 KiB in front of 100 KiB of text: bitmap word 0 lies in the range of three workgroups, the corpus reports the
    clearing path, and the kernels that merge with atomics run - in both flush forms."""
    rng = np.random.default_rng(6)
    long_line = np.frombuffer(filler, dtype=np.uint8)[rng.integers(0, len(filler), size=600 * 1024)].tobytes()
    tail = synthetic(kind, 13, 100 * 1024).tobytes()
    data = np.frombuffer(tail[:tail.find(b"\n") + 1] + long_line + b"\n" + tail, dtype=np.uint8).copy()
    want = OracleRegex(p).match_lines(data)
    assert 0 < int(want.sum()) < len(want)
    corpus = rr.Corpus(torch.from_numpy(data).cuda(), stripe=512)
    assert not corpus.one_launch and (len(data) + 511) // 512 > 1024
    both_flush_forms(p, lambda r: r.match_corpus_bits, corpus, want, ("long line", kind))


def high_byte_corpus(long_line):
    """URL text for the contains table of HOSTS with bytes >= 0x80 put in: in front of a line, behind it, inside it (the verdict
    is then the OR over the two halves: such a byte is ordinary text no pattern takes) and lines of such bytes only."""
    rng = np.random.default_rng(8)
    lines = split_lines(synthetic("url", 14, 150 * 1024).tobytes())
    if long_line:
        filler = np.frombuffer(b"hftp:/.az", dtype=np.uint8)
        lines.insert(3, filler[rng.integers(0, len(filler), size=600 * 1024)].tobytes())
    asc = dot_star(HOSTS, lines)
    want = list(asc)
    for i in range(5, len(lines), 7):
        ln, kind, hi = lines[i], (i // 7) % 4, [b"\x80", b"\xc3\xa9", b"\xff", b"\xe2\x82\xac"][(i // 7) % 4]
        if len(ln) > 100000:
            continue
        if kind == 0:
            lines[i] = hi + ln
        elif kind == 1:
            lines[i] = ln + hi
        elif kind == 2:
            cut = int(rng.integers(0, len(ln) + 1))
            lines[i] = ln[:cut] + hi + ln[cut:]
            want[i] = int(dot_star(HOSTS, [ln[:cut], ln[cut:]]).any())
        else:
            lines[i] = hi * int(rng.integers(1, 9))
            want[i] = 0
    data = np.frombuffer(b"\n".join(lines) + b"\n", dtype=np.uint8).copy()
    high = np.nonzero(data >= 0x80)[0]
    assert (high % 2 == 0).any() and (high % 2 == 1).any()
    return data, np.array(want, dtype=np.uint8)


@pytest.mark.parametrize("long_line", (False, True))
def test_high_bytes_through_the_contains_kernel(long_line):
    data, want = high_byte_corpus(long_line)
    assert 0 < int(want.sum()) < len(want)
    corpus = rr.Corpus(torch.from_numpy(data).cuda(), stripe=512)
    assert corpus.one_launch == (not long_line)
    both_flush_forms(HOSTS, lambda r: r.contains_corpus_bits, corpus, want, ("contains", long_line))


def edge_lines(accepted):
    """Lines with 0x00 and 0x7f inside an otherwise accepted line, single-byte lines of them, and empty lines."""
    out = []
    for b in (b"\x00", b"\x7f"):
        for ln in accepted[:3]:
            out += [b + ln, ln + b, ln[:7] + b + ln[7:], ln[:8] + b + ln[8:], b, b + b, b""]
    return out


@pytest.mark.parametrize("p,kind", [(U2, "url"), (PAIRS, "pairs")])
def test_edges_of_the_pair_step(p, kind):
    """The special bytes on either byte of a pair (each line is placed once at an even and once at an odd offset), an accepted line
    across the workgroup end, then the same corpus with and without its last '\\n', even and odd in length."""
    o = OracleRegex(p)
    base = synthetic(kind, 15, 560 * 1024).tobytes()
    base = base[:base.rfind(b"\n") + 1]
    accepted = [ln for ln in split_lines(base[:64 * 1024]) if 24 <= len(ln) <= 200 and o.accepts(ln.decode("latin-1"))]
    assert len(accepted) >= 3
    straddle = accepted[0]
    at = WG_BYTES - len(straddle) // 2 - 1
    base = base[:at] + b"\n" + straddle + b"\n" + base[at + len(straddle) + 2:]
    special = b""
    for ln in edge_lines(accepted):
        for parity in (0, 1):
            if (len(base) + len(special)) % 2 != parity:
                special += b"\n"                                     # an empty line shifts the parity
            special += ln + b"\n"
    for tail in (b"", b"\n", accepted[1], accepted[1] + b"a", b"\x00", b"\x7f\x7f"):
        data = np.frombuffer(base + special + tail, dtype=np.uint8).copy()
        assert data[WG_BYTES - 1] != 10 and data[WG_BYTES] != 10
        for b in (0x00, 0x7f):
            where = np.nonzero(data == b)[0]
            assert (where % 2 == 0).any() and (where % 2 == 1).any()
        want = o.match_lines(data)
        lines = split_lines(data.tobytes())
        assert want[lines.index(straddle, 1000)] == 1
        corpus = rr.Corpus(torch.from_numpy(data).cuda(), stripe=512)
        assert corpus.one_launch
        run_dirty(regex(p).match_corpus_bits, corpus, want, what=(kind, "tail", tail[:8], len(data) % 2))
    seen = {len(base + special + t) % 2 for t in (b"", b"\n", accepted[1], accepted[1] + b"a", b"\x00", b"\x7f\x7f")}
    assert seen == {0, 1}


@pytest.mark.parametrize("p,texts", [
    (U2, [b"http://ab.cd\nftp://x.yz/q", b"http://ab.cd\nftp://x.yz/q\n", b"ftp://a.bc", b"\n", b"\n\n", b"x", b"ftp://a.b\x00\nhttp://ab.cd/\x7f\nftp://a.bc\n\n",
          b"http://example.com/a/b/c?d=e#f\n" * 4]),
    (A300, [b"a", b"a\n", b"aa\nb\n\naaa", b"a" * 127, b"a" * 126 + b"\n", b"\x00a\na\x00\n\x7f\na\x7fa\naa\n", b"a" * 60 + b"\n" + b"a" * 66])])
def test_corpora_shorter_than_one_round(p, texts):
    """Fewer than 128 bytes: no whole round, every pair goes through the tail step, the odd last byte through the virtual '\\n'."""
    o = OracleRegex(p)
    r = regex(p)
    for k, t in enumerate(texts):
        assert 0 < len(t) < 128
        data = np.frombuffer(t, dtype=np.uint8).copy()
        corpus = rr.Corpus(torch.from_numpy(data).cuda(), stripe=512)
        run_dirty(r.match_corpus_bits, corpus, o.match_lines(data), fill=FILLS[k & 3], what=("short", t[:16]))
