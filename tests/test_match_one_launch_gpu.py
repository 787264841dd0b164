"""The stride-2 table kernel as ONE launch (no clear of the bitmap in front of it) and its two flush forms, against the oracle.
Every call here runs over a DIRTY bitmap: a word the kernel does not store, or merges into what it finds, shows at once.  The
cases are the ones at which the write-out takes another path: one workgroup and several, the shared word between two workgroups
with 0, 1 and 31 lines of the first one in it, lines longer than a workgroup's text (three writers per word: the corpus reports
the clearing path), more result words per workgroup than the LDS window holds, the last workgroup's tail, both kernels (plain /
bytes >= 0x80), and every flush period in its compile-time or per-launch form."""
import random

import numpy as np
import pytest

import roaringregex_amd as rr
from contains_cases import dot_star, long_ascii_lines
from patterns import U2
from pyoracle import OracleRegex

torch = pytest.importorskip("torch")
from dirty_bitmap import FILLS, run_dirty  # noqa: E402  (it imports torch)

pytestmark = pytest.mark.gpu

ABB = "(a|b)*abb(a|b)*"
WG_STRIPES = 1024                          # stripes per workgroup of the batch kernel


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"


def ab_lines(rng, nbytes, mean):
    """About nbytes of a/b lines with `mean` bytes per line, newline included."""
    a = np.frombuffer(b"ab\n", dtype=np.uint8)
    q = 1.0 / mean
    return a[rng.choice(3, size=nbytes, p=[(1 - q) / 2, (1 - q) / 2, q])].copy()


@pytest.fixture(scope="module")
def url_1mib():
    import synth
    data = synth.corpus("url", 5, 1 << 20)
    want = OracleRegex(U2).match_lines(data)
    corpus = rr.Corpus(torch.from_numpy(data).cuda(), stripe=512)
    assert corpus.stripe == 512 and (corpus.num_bytes + 511) // 512 == 2 * WG_STRIPES       # two workgroups
    return corpus, want


def test_dirty_bitmap(url_1mib):
    corpus, want = url_1mib
    r = rr.RRegex(U2)
    r.set_background_order(False)
    assert r.engine_name == "dfa-stride2-table" and corpus.one_launch and 0 < corpus.one_launch_span < 1024
    run_dirty(r.match_corpus_bits, corpus, want, what="url")


def test_slots_are_zero_again_after_every_launch(url_1mib):
    """Three launches in a row on one stream, then one on a second stream, each over another dirty fill."""
    corpus, want = url_1mib
    r = rr.RRegex(U2)
    r.set_background_order(False)
    first, second = torch.cuda.Stream(), torch.cuda.Stream()
    for k, stream in enumerate((first, first, first, second)):
        run_dirty(r.match_corpus_bits, corpus, want, fill=FILLS[k], stream=stream, what="launch %d" % k)
    run_dirty(r.match_corpus_bits, corpus, want, fill=FILLS[1], what="current stream")


def boundary_corpus(rng, lines_mod_32, fresh):
    """A corpus of two workgroups at stripe 512 with `lines_mod_32` (mod 32) line ends in front of the second one's first stripe,
    which begins a line (fresh) or lies inside one."""
    cut = WG_STRIPES * 512
    head = ab_lines(rng, cut - 400, 24).tobytes()
    head = head[:head.rfind(b"\n") + 1]
    n = head.count(b"\n") + 1                                       # (+ 1: the filler line below)
    head += b"ab\n" * ((lines_mod_32 - n) % 32)
    fill = cut - len(head)
    assert fill > 64
    if fresh:
        head += b"a" * (fill - 5) + b"abba\n"                       # ends exactly at the cut
    else:
        head += b"b" * fill                                         # goes on behind the cut ...
    tail = (b"" if fresh else b"bbbabb\n") + ab_lines(rng, 100_000, 24).tobytes()
    data = np.frombuffer(head + tail, dtype=np.uint8).copy()
    if fresh:
        assert data[cut - 1] == 10
    assert int((data[:cut] == 10).sum()) % 32 == (lines_mod_32 if fresh else (lines_mod_32 - 1) % 32)
    return data


@pytest.mark.parametrize("fresh", (True, False))
def test_boundary_word_between_two_workgroups(fresh):
    """0, 1 and 31 (mod 32) lines in front of the second workgroup's first stripe - with the line that straddles the cut, which
    the first workgroup reports, the first workgroup holds 0 ... 32 bits of the shared word - and a corpus of one workgroup."""
    rng = np.random.default_rng(4 + fresh)
    o = OracleRegex(ABB)
    r = rr.RRegex(ABB)
    assert r.engine_name == "dfa-stride2-table"
    for k in (0, 1, 31, 32):
        data = boundary_corpus(rng, k % 32, fresh)
        corpus = rr.Corpus(torch.from_numpy(data).cuda(), stripe=512)
        assert corpus.one_launch and WG_STRIPES < (len(data) + 511) // 512 <= 2 * WG_STRIPES
        run_dirty(r.match_corpus_bits, corpus, o.match_lines(data), fill=FILLS[k & 3], what=("boundary", k, fresh))
    for n in (200_000, 77):                                          # one workgroup: its first word and the tail are its own
        data = ab_lines(rng, n, 24)
        corpus = rr.Corpus(torch.from_numpy(data).cuda(), stripe=512)
        assert corpus.one_launch
        run_dirty(r.match_corpus_bits, corpus, o.match_lines(data), what=("single", n))


def test_lines_longer_than_a_workgroup_take_the_clearing_path():
    """Lines of 600 KiB at stripe 512 (a workgroup's text: 512 KiB), five workgroups: bitmap word 0 lies in the range of all of
    them, the corpus says so, and the call clears and merges as before."""
    rng = np.random.default_rng(9)
    lines = []
    for k in range(4):
        ln = np.frombuffer(b"ab", dtype=np.uint8)[rng.integers(0, 2, size=600 * 1024)].copy()
        if k % 2:
            ln[:] = ord("a")                                         # no abb
        lines.append(ln.tobytes())
    data = np.frombuffer(b"\n".join(lines) + b"\nabb\nab\n", dtype=np.uint8).copy()
    corpus = rr.Corpus(torch.from_numpy(data).cuda(), stripe=512)
    assert (len(data) + 511) // 512 > 3 * WG_STRIPES
    assert not corpus.one_launch and corpus.one_launch_span == 0
    r = rr.RRegex(ABB)
    want = OracleRegex(ABB).match_lines(data)
    assert list(want) == [1, 0, 1, 0, 1, 0]
    run_dirty(r.match_corpus_bits, corpus, want, what="long lines")
    run_dirty(r.contains_corpus_bits, corpus, want, what="long lines, contains")


def test_more_result_words_than_the_window_holds():
    """2-byte lines at stripe 2048: a workgroup's 2 MiB hold a million lines, 32768 bitmap words, and no table leaves a window
    of more than 11776.  The words beyond the window go to memory one by one: that launch keeps its clear."""
    rng = np.random.default_rng(10)
    n = 2_200_000
    data = np.empty(2 * n, dtype=np.uint8)
    data[0::2] = np.frombuffer(b"ab", dtype=np.uint8)[rng.integers(0, 2, size=n)]
    data[1::2] = 10
    corpus = rr.Corpus(torch.from_numpy(data).cuda(), stripe=2048)
    assert corpus.stripe == 2048 and (len(data) + 2047) // 2048 > 2 * WG_STRIPES
    assert corpus.one_launch and corpus.one_launch_span >= 32768
    r = rr.RRegex("a")
    assert r.engine_name == "dfa-stride2-table"
    want = (data[0::2] == ord("a")).astype(np.uint8)
    assert (OracleRegex("a").match_lines(data[:20000]) == want[:10000]).all()
    run_dirty(r.match_corpus_bits, corpus, want, what="2-byte lines")


@pytest.mark.parametrize("mean", (5, 20, 48, 200))
def test_flush_forms(mean):
    """The automatic period and every explicit one, 1 MiB each: 32 runs the kernel with the period compiled in, the others the
    one that takes it per launch; the bits are the oracle's every time."""
    rng = np.random.default_rng(100 + mean)
    data = ab_lines(rng, 1 << 20, mean)
    want = OracleRegex(ABB).match_lines(data)
    corpus = rr.Corpus(torch.from_numpy(data).cuda())
    assert corpus.one_launch
    for slots in (0, 1, 2, 4, 8, 16, 32):
        r = rr.RRegex(ABB)
        assert r.engine_name == "dfa-stride2-table"
        r.set_flush_slots(slots)
        period, compiled_in = r.flush_slots(corpus)
        if slots:
            assert (period, compiled_in) == (slots, slots == 32)
        else:                                                        # automatic: a full period from 33 bytes per line on
            assert compiled_in == (period == 32) and (period == 32) == (mean >= 33), (mean, period)
        run_dirty(r.match_corpus_bits, corpus, want, fill=FILLS[slots & 3], what=("flush", mean, slots))


def test_high_bytes_through_contains():
    """rrx_contains_corpus on a corpus with bytes >= 0x80: the kernel that steps them as 0x00, two workgroups, a dirty bitmap."""
    rng = random.Random(12)
    p = "ab+c"
    lines = long_ascii_lines(rng, p, 1500, maxlen=900)
    want = list(dot_star(p, lines))
    for at, ln in ((1100, b"\xc3\xa9\xff"), (400, b"\x80"), (0, b"\xe2\x82\xac")):      # lines of high bytes only: no match
        lines.insert(at, ln)
        want.insert(at, 0)
    data = np.frombuffer(b"\n".join(lines) + b"\n", dtype=np.uint8).copy()
    corpus = rr.Corpus(torch.from_numpy(data).cuda(), stripe=512)
    assert (len(data) + 511) // 512 > WG_STRIPES and corpus.one_launch
    r = rr.RRegex(p)
    assert r.contains_engine_name == "dfa-stride2-table"
    run_dirty(r.contains_corpus_bits, corpus, np.array(want, dtype=np.uint8), what="contains, high bytes")
