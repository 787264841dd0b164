"""The group, wave and sparse NFA engines in every instantiation the front end reaches, on the GPU, against the closed forms of
coop_engine_cases.py (test_coop_engines_lowering.py shows on the CPU which kernel each case launches, that the closed forms are the
oracle's language and that the lines notice one wrong step of a kernel): match_stripes_group_kernel / match_extents_group_kernel<G, K,
MODE, SLOT0>, match_stripes_wave_kernel / match_extents_wave_kernel<WL, FRONT>, match_stripes_sparse_kernel /
match_extents_sparse_kernel<WR, LROWS> through every entry, bit for bit."""
import numpy as np
import pytest

import coop_engine_cases as T
import roaringregex_amd as rr

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD = 64                                                 # poisoned elements on either side of an output buffer
POISON = {torch.uint8: 0xa5, torch.int32: 0x5a5a5a5a}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"


def to_dev(data):
    return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()


def bits_to_bytes(words, n):
    w = words.cpu().numpy().view(np.uint32)
    return ((w[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1).astype(np.uint8).reshape(-1)[:n]


class Guarded:
    """an output buffer of n elements between two runs of poisoned guard elements"""

    def __init__(self, n, dtype):
        self.n, self.poison = n, POISON[dtype]
        self.whole = torch.full((n + 2 * GUARD,), self.poison, dtype=dtype, device="cuda")
        self.out = self.whole[GUARD:GUARD + n]

    def intact(self):
        w = self.whole.cpu().numpy()
        return bool((w[:GUARD] == self.poison).all() and (w[GUARD + self.n:] == self.poison).all())


def same(case, got, want, lines, entry, stripe="-", guard=None):
    where = "%s: %s, %s, stripe %s" % (case.pattern[:60], case.inst, entry, stripe)
    assert guard is None or guard.intact(), where + ": wrote outside its output buffer"
    assert got.shape == want.shape, (where, got.shape, want.shape)
    bad = np.nonzero(got != want)[0]
    if bad.size:
        i = int(bad[0])
        raise AssertionError("%s: line %d (of %d wrong among %d, %d bytes) got %d want %d" % (where, i, bad.size, len(want), len(lines[i]), int(got[i]), int(want[i])))


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id)
def test_coop_engine_case(case):
    lines, want = T.lines(case), T.expected(case)
    n = len(want)
    r = rr.RRegex(case.pattern, T.ENGINE_OF[case.engine])
    assert r.engine_name == T.ENGINE_NAME[case.engine] and r.words_per_set == (case.nbits + 31) // 32, (case.id, r.engine_name, r.words_per_set)
    for final_newline in (True, False):
        dev = to_dev(T.corpus(case, final_newline))
        tail = "final newline" if final_newline else "no final newline"
        for stripe in (1024, 16384, 0):
            corpus = rr.Corpus(dev, stripe=stripe)
            assert corpus.num_lines == n
            g = Guarded(n, torch.uint8)
            same(case, r.match_corpus(corpus, out=g.out).cpu().numpy(), want, lines, "match_corpus, " + tail, corpus.stripe, g)
        g = Guarded((n + 31) // 32, torch.int32)
        bits, nlines = r.match_device_bits(dev, cap_lines=n, out=g.out)
        assert nlines == n
        same(case, bits_to_bytes(bits, nlines), want, lines, "match_device_bits, " + tail, guard=g)
    # a corpus that does not begin where its allocation does (sixteen bytes in: a corpus base is 16-byte aligned)
    data = T.corpus(case)
    inner = torch.cat([torch.full((16,), 10, dtype=torch.uint8, device="cuda"), to_dev(data)])[16:]
    same(case, r.match_corpus(rr.Corpus(inner, stripe=1024)).cpu().numpy(), want, lines, "match_corpus, sixteen bytes into its allocation", 1024)
    # the extents kernels: the same lines as explicit items, squeezed together and with a separator byte each
    lens = np.array([len(t) for t in lines], dtype=np.int64)
    off0 = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)])).cuda()
    off1 = torch.from_numpy(np.concatenate([[0], np.cumsum(lens + 1)])).cuda()
    g = Guarded(n, torch.uint8)
    same(case, r.match_extents(to_dev(b"".join(lines)), off0, out=g.out).cpu().numpy(), want, lines, "match_extents, trim 0", guard=g)
    sep = to_dev(data)
    g = Guarded(n, torch.uint8)
    same(case, r.match_extents(sep, off1, trim=1, out=g.out).cpu().numpy(), want, lines, "match_extents, trim 1", guard=g)
    odd = torch.cat([torch.zeros(1, dtype=torch.uint8, device="cuda"), sep])[1:]
    assert odd.data_ptr() % 16 == 1
    g = Guarded(n, torch.uint8)
    same(case, r.match_extents(odd, off1, trim=1, out=g.out).cpu().numpy(), want, lines, "match_extents, trim 1, base one byte off 16-byte alignment", guard=g)
    g = Guarded(n, torch.uint8)
    same(case, r.match_items(rr.Items(sep, off1, trim=1), out=g.out).cpu().numpy(), want, lines, "match_items", guard=g)
    # the facade, one string per call
    for i in T.edge_lines(case):
        got = r.get_acceptance_iter(lines[i]).advance().value() is not None
        assert got == bool(want[i]), (case.pattern[:60], case.inst, "facade", "line", i, len(lines[i]))
