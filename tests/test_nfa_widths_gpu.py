"""The NFA lane engine at every width and in every build, on the GPU, against the oracle (case table and vectors: nfa_width_cases.py;
test_nfa_widths_lowering.py shows on the CPU which kernel each case reaches and that the vectors are the oracle's): the batch kernels
match_stripes_nfa (LineNfaEngine<W, SELF, RULES, CARRY>, 8 widths x 4 builds), the one-pass kernels match_onepass_nfa (8 x 3), the
extents kernel and the facade on PlainNfaEngine<W>, and the sampled table's two recheck kernels at four program widths."""
import numpy as np
import pytest

import nfa_width_cases as T
import roaringregex_amd as rr
from pyoracle import OracleRegex

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LANES = 1024                                               # device.hpp: kThreads, stripes per workgroup
BUILD = {"chain": "<W,0,0,0>", "self": "<W,1,0,0>", "carry": "<W,1,0,1>", "exc": "<W,1,1,0> carry flag off", "mix": "<W,1,1,0> carry flag on"}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"


def to_dev(data):
    return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()


def bits_to_bytes(words, n):
    w = words.cpu().numpy().view(np.uint32)
    return ((w[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1).astype(np.uint8).reshape(-1)[:n]


def same(case, got, want, lines, entry, stripe="-"):
    assert got.shape == want.shape, (case.pattern, entry, stripe, got.shape, want.shape)
    bad = np.nonzero(got != want)[0]
    if bad.size:
        i = int(bad[0])
        raise AssertionError("%s: program W %d, kernel W %d, build %s, %s, stripe %s: line %d (of %d wrong among %d, %d bytes) got %d want %d" % (
            case.pattern, case.W, T.kernel_width(case.W), BUILD[case.shape], entry, stripe, i, bad.size, len(want), len(lines[i % len(lines)]),
            int(got[i]), int(want[i])))


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id)
def test_lane_engine_width_case(case):
    lines, want = T.lines(case), T.expected(case)
    r = rr.RRegex(case.pattern, rr.ENGINE_NFA)
    assert r.engine_name == "nfa-shift-and" and r.words_per_set == case.W
    for final_newline in (True, False):
        dev = to_dev(T.corpus(case, final_newline))
        tail = "final newline" if final_newline else "no final newline"
        for stripe in (1024, 16384, 0):
            corpus = rr.Corpus(dev, stripe=stripe)
            assert corpus.num_lines == len(want)
            same(case, r.match_corpus(corpus).cpu().numpy(), want, lines, "match_corpus, " + tail, corpus.stripe)
        bits, nlines = r.match_device_bits(dev)
        assert nlines == len(want)
        same(case, bits_to_bytes(bits, nlines), want, lines, "match_device_bits, " + tail)
    # a corpus that does not begin where its allocation does (sixteen bytes in: a corpus base is 16-byte aligned, rrx_corpus_create
    # refuses any other - test_corpus_base_one_byte_into_an_allocation_is_refused)
    data = T.corpus(case)
    inner = torch.cat([torch.full((16,), 10, dtype=torch.uint8, device="cuda"), to_dev(data)])[16:]
    same(case, r.match_corpus(rr.Corpus(inner, stripe=1024)).cpu().numpy(), want, lines, "match_corpus, sixteen bytes into its allocation", 1024)
    # more than one workgroup (1024 stripes each) at stripe 1024: the corpus over and over
    reps = (LANES * 1024) // len(data) + 2
    big, want_big = to_dev(data * reps), np.tile(want, reps)
    corpus = rr.Corpus(big, stripe=1024)
    assert corpus.stripe == 1024 and len(data) * reps > LANES * 1024 and corpus.num_lines == len(want_big)
    same(case, r.match_corpus(corpus).cpu().numpy(), want_big, lines, "match_corpus, %d workgroups" % -(-len(data) * reps // (LANES * 1024)), 1024)
    bits, nlines = r.match_device_bits(big)
    assert nlines == len(want_big)
    same(case, bits_to_bytes(bits, nlines), want_big, lines, "match_device_bits, the corpus %d times" % reps)
    # PlainNfaEngine<W>: the same lines as explicit items, squeezed together and with a separator byte each
    lens = np.array([len(t) for t in lines], dtype=np.int64)
    off0 = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)])).cuda()
    off1 = torch.from_numpy(np.concatenate([[0], np.cumsum(lens + 1)])).cuda()
    same(case, r.match_extents(to_dev(b"".join(lines)), off0).cpu().numpy(), want, lines, "match_extents, trim 0")
    sep = to_dev(data)
    same(case, r.match_extents(sep, off1, trim=1).cpu().numpy(), want, lines, "match_extents, trim 1")
    odd = torch.cat([torch.zeros(1, dtype=torch.uint8, device="cuda"), sep])[1:]
    assert odd.data_ptr() % 16 == 1
    same(case, r.match_extents(odd, off1, trim=1).cpu().numpy(), want, lines, "match_extents, trim 1, one byte into its allocation")
    # the facade, one string per call, on the lines of the edge lengths
    for i in T.edge_lines(case)[:12]:
        if b"\x00" in lines[i]:
            continue                                       # (a C string ends there)
        got = r.get_acceptance_iter(lines[i]).advance().value() is not None
        assert got == bool(want[i]), (case.pattern, "program W", case.W, "kernel W", T.kernel_width(case.W), "facade", "line", i, len(lines[i]))


def test_corpus_base_one_byte_into_an_allocation_is_refused():
    """rrx_corpus_create and rrx_match_device take a 16-byte aligned base (the batch kernels load sixteen bytes at a time) and say so;
    rrx_match_extents takes any (test_lane_engine_width_case runs it one byte in)."""
    dev = to_dev(b"a\nb\n" * 64)
    with pytest.raises(rr.RRegexError, match="16-byte aligned"):
        rr.Corpus(dev[1:])
    with pytest.raises(rr.RRegexError, match="16-byte aligned"):
        rr.RRegex("a", rr.ENGINE_NFA).match_device_bits(dev[1:])


@pytest.mark.parametrize("n,W", T.SAMPLED_CASES, ids=lambda v: str(v))
def test_sampled_table_rechecks_escaped_lines_at_this_width(n, W):
    """recheck_lines_kernel<W> and recheck_escaped_kernel<W> (the NFA engine deciding the lines a sampled table could not) at a padded
    and an exact six words, twelve and a padded sixteen: a corpus with a dozen escaping lines - the first and the last line, one that
    starts at a stripe boundary, one longer than a stripe - takes the list kernel, one with more escaping lines than the list holds
    takes the walk over the stripes.  Exact against the oracle, equal to the same regex without its table, and the number of lines
    that escaped is the number built in (test_nfa_widths_lowering.py: exactly those lines escape from the table)."""
    pattern = T.sampled_pattern(n)
    o = OracleRegex(pattern)
    plain = rr.RRegex(pattern)
    plain.set_sampled_table(False)
    assert plain.engine_name == "nfa-shift-and" and plain.words_per_set == W

    def run(name, data, escaping, stripes):
        r = rr.RRegex(pattern)                               # (a table of its own per corpus: a launch is judged on the launch before it)
        assert r.learn_table(T.sampled_sample()) is not None
        arr = np.frombuffer(data, dtype=np.uint8)
        want = o.match_lines(arr)
        assert want[escaping].any() and not want[escaping].all() and not np.delete(want, escaping).any()
        dev = torch.from_numpy(arr.copy()).cuda()
        cap = T.sampled_list_capacity(len(want))
        for stripe in stripes:
            corpus = rr.Corpus(dev, stripe=stripe)
            assert corpus.stripe == (stripe or corpus.stripe) and corpus.num_lines == len(want)
            got = r.match_corpus(corpus).cpu().numpy()
            escapes = r.sampled_escapes()
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, (pattern, "program W", W, "kernel W", T.kernel_width(W), name, "stripe", stripe, "first bad line", int(bad[0]),
                                   "escaping" if int(bad[0]) in escaping else "decided by the table", "escapes", escapes, "list capacity", cap)
            assert escapes == len(escaping), (name, stripe, escapes, len(escaping))
            assert (escapes <= cap) == (name == "list"), (name, escapes, cap)
            assert escapes * 100 <= len(want) * T.SAMPLED_RETIRE_PERCENT
            assert torch.equal(plain.match_corpus_bits(corpus), r.match_corpus_bits(corpus)), (name, stripe)
            torch.cuda.synchronize()
            assert r.sampled_table is not None and not r.sampled_table_retired, (name, stripe)

    for stripe in (1024, 4096):
        data, escaping, boundary = T.sampled_few(n, stripe)
        assert data[:data.index(b"\n") + 1].count(b"\n") == 1 and sum(len(t) + 1 for t in data.split(b"\n")[:boundary]) % stripe == 0
        run("list", data, escaping, (stripe,))
    data, escaping = T.sampled_many(n)
    run("walk", data, escaping, (1024, 0))
