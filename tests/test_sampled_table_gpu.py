"""The sampled-table match path on the GPU, stage by stage, against the oracle (case table: sampled_table_cases.py;
test_sampled_table_lowering.py shows on the CPU that every case has the property it is named for and that exactly the lines built to
escape leave the table): match_stripes2_two_bit_kernel (A1 ... A5), split_two_bit_kernel (B1 ... B3), the hand-over between
recheck_lines_kernel and recheck_escaped_kernel at the cap (C), and where each of the two finds the first byte of an escaped line (D, E).
Every launch that is checked has a regex and a table of its own (a launch is judged on the one before it), writes into a bitmap that
was filled with a pattern and is longer than the corpus needs, and is held against the oracle, against the same regex without its
table, and against the number of lines that must have escaped."""
import numpy as np
import pytest

import roaringregex_amd as rr
import sampled_table_cases as T
from pyoracle import OracleRegex

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FILLS = (-1, 0x55555555, -0x21524111, 0x7FFFFFFF)          # (0xFFFFFFFF, ..., 0xDEADBEEF as int32)
GUARD_WORDS = 8


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"


@pytest.fixture(scope="module")
def refs():
    """(the oracle, the regex without its table): shared, never changed"""
    plain = rr.RRegex(T.PATTERN)
    plain.set_sampled_table(False)
    assert plain.engine_name == "nfa-shift-and" and plain.words_per_set == 2
    return OracleRegex(T.PATTERN), plain


def learnt():
    r = rr.RRegex(T.PATTERN)
    assert r.learn_table(T.sample()) is not None
    return r


def words_of(want, nwords):
    bits = np.zeros(nwords * 32, dtype=np.uint8)
    bits[:len(want)] = want
    return np.packbits(bits, bitorder="little").view(np.uint32)


def bits_to_bytes(host_words, n):
    return np.unpackbits(host_words.view(np.uint8), bitorder="little")[:n]


def same(case, stripe, entry, got, want, escaping):
    bad = np.nonzero(got != want)[0]
    if bad.size:
        i = int(bad[0])
        where = np.searchsorted(escaping, i)
        escapes = where < len(escaping) and int(escaping[where]) == i
        raise AssertionError("%s, stripe %s, %s: line %d (%s; %d wrong of %d) got %d want %d" % (
            case.id, stripe, entry, i, "ESCAPES" if escapes else "decided by the table", bad.size, len(want), int(got[i]), int(want[i])))


def check(case, refs):
    o, plain = refs
    b = T.built(case)
    want = T.expected(case, o)
    nlines, nw = len(want), (len(want) + 31) // 32
    want_words = words_of(want, nw)
    dev = torch.from_numpy(b.data.copy()).cuda()
    cap = T.list_capacity(nlines)
    for k, stripe in enumerate(case.stripes):
        r = learnt()                                         # (a table of its own per launch checked: a launch is judged on the one before it)
        corpus = rr.Corpus(dev, stripe=stripe)
        assert corpus.stripe == (stripe or corpus.stripe) and corpus.num_lines == nlines, (case.id, stripe, corpus.num_lines, nlines)
        got = r.match_corpus(corpus).cpu().numpy()
        escapes = r.sampled_escapes()
        same(case, corpus.stripe, "match_corpus", got, want, b.escaping)
        assert escapes == len(b.escaping), (case.id, corpus.stripe, "escaped", escapes, "built to escape", len(b.escaping))
        assert (escapes <= cap) == (case.path == "list"), (case.id, escapes, cap)
        # the bitmap itself, over a dirty one with words behind it: every word the oracle's, the guard untouched; equal to the regex without its table
        fill = FILLS[k & 3]
        out = torch.full((nw + GUARD_WORDS,), fill, dtype=torch.int32, device="cuda")
        bits = r.match_corpus_bits(corpus, out=out)
        assert bits.numel() == nw
        host = out.cpu().numpy().view(np.uint32)
        same(case, corpus.stripe, "match_corpus_bits", bits_to_bytes(host[:nw].copy(), nlines), want, b.escaping)
        assert np.array_equal(host[:nw], want_words), (case.id, corpus.stripe, "bits behind the last line")
        assert (host[nw:] == np.uint32(fill & 0xFFFFFFFF)).all(), (case.id, corpus.stripe, "words behind the bitmap were written")
        assert torch.equal(plain.match_corpus_bits(corpus), bits), (case.id, corpus.stripe, "the regex without its table")
        assert r.sampled_escapes() == len(b.escaping)
        torch.cuda.synchronize()
        assert r.sampled_table is not None and not r.sampled_table_retired, (case.id, corpus.stripe)
    r = learnt()
    bits, n = r.match_device_bits(dev)
    assert n == nlines, (case.id, "match_device_bits", n, nlines)
    same(case, "-", "match_device_bits", bits_to_bytes(bits.cpu().numpy().view(np.uint32)[:nw].copy(), nlines), want, b.escaping)
    assert r.sampled_table is not None and not r.sampled_table_retired, (case.id, "match_device_bits")


@pytest.mark.parametrize("group", T.GROUPS)
def test_sampled_table_cases(group, refs):
    """A1 dense line ends, A2 the corpus tail, A3 the follow path, A4 the wide word two workgroups share, A5 the window overflow; B1
    bitmap sizes, B2 the flush inside a turn, B3 the second turn; C the escaped total at the cap; D the list kernel's line-start search;
    E the walk over the stripes."""
    cases = T.of_group(group)
    assert cases
    for case in cases:
        check(case, refs)


def test_two_corpora_on_two_side_streams_back_to_back(refs):
    """One regex and its table, two corpora of the same number of lines (a launch is judged on the escapes of the one before it: one
    escaped total below the cap, decided through the list, one above it, decided by the walk), two side streams, launches back to back
    without a host synchronisation in between: the scratch of the sampled launch (wide bitmap, escaped bitmap, list) is the regex' and is
    handed from one launch to the next in order, so every result is its own corpus' and exact."""
    o, _ = refs
    picked = [c for c in T.CASES if c.id in ("C-1024-1023", "C-1024-1025")]
    assert [c.path for c in picked] == ["list", "walk"]
    r = learnt()
    corpora, wants = [], []
    for case in picked:
        b = T.built(case)
        corpora.append(rr.Corpus(torch.from_numpy(b.data.copy()).cuda(), stripe=512))
        wants.append(words_of(T.expected(case, o), (len(b.idx) + 31) // 32))
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    rounds = 4
    outs = [[torch.full((len(w) + GUARD_WORDS,), FILLS[it & 3], dtype=torch.int32, device="cuda") for it in range(rounds)] for w in wants]
    torch.cuda.synchronize()
    for it in range(rounds):
        for k in (0, 1):
            r.match_corpus_bits(corpora[k], out=outs[k][it], stream=streams[k])
    torch.cuda.synchronize()
    for k in (0, 1):
        for it in range(rounds):
            host = outs[k][it].cpu().numpy().view(np.uint32)
            nw = len(wants[k])
            bad = np.nonzero(host[:nw] != wants[k])[0]
            assert bad.size == 0, (picked[k].id, "launch", it, "word", int(bad[0]), hex(int(host[bad[0]])), hex(int(wants[k][bad[0]])))
            assert (host[nw:] == np.uint32(FILLS[it & 3] & 0xFFFFFFFF)).all(), (picked[k].id, it, "words behind the bitmap were written")
    assert r.sampled_table is not None and not r.sampled_table_retired
