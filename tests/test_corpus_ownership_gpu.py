"""What a corpus owns besides its line index, against the oracle, each from its first use to the corpus' end: the search chunk
index where it IS the stripe index (stripe 16384, the search kernel's chunk) and where it is an index of its own (stripe 1024), the
line offsets and the per-call scratch of a pattern that accepts the empty string, the exchange slot arrays of the one-launch
stride-2 kernel (one per stream), and the second index of a corpus whose automatic stripe changes once its lines are counted."""
import random

import numpy as np
import pytest

import roaringregex_amd as rr
from patterns import U2
from pyoracle import OracleRegex

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ABB = "(a|b)*abb(a|b)*"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"


@pytest.fixture(scope="module")
def text_64k():
    """64 KiB of short lines (four chunks of the search kernel) and the oracle's searches of it, per pattern."""
    rng = random.Random(21)
    lines, size = [], 0
    while size < 65536:
        lines.append("".join(rng.choice("abc") for _ in range(rng.choice([0, 1, 2, 5, 9, 14, 22]))).encode())
        size += len(lines[-1]) + 1
    data = (b"\n".join(lines) + b"\n")[:65535] + b"\n"
    want = {}
    for p in ("ab+c", "b*"):                   # search tables / accepts "": line offsets, no chunk index
        o = OracleRegex(p)
        want[p] = (o.search_lines(data), o.search_all(data))
    return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda(), want


@pytest.mark.parametrize("stripe", [16384, 1024])
@pytest.mark.parametrize("pattern", ["ab+c", "b*"])
def test_search_then_free(text_64k, stripe, pattern):
    dev, want = text_64k
    (ws, we), (wc, was, wae) = want[pattern]
    corpus = rr.Corpus(dev, stripe=stripe)
    assert corpus.stripe == stripe and corpus.num_bytes == 65536 and corpus.num_lines == len(ws)
    r = rr.RRegex(pattern)
    for _ in range(2):                         # (the second round finds everything built)
        st, en = r.search_corpus(corpus)
        assert (st.cpu().numpy() == ws).all() and (en.cpu().numpy() == we).all()
        cnt, first, ast, aen = r.search_all(corpus)
        assert (cnt.cpu().numpy() == wc.astype(np.int32)).all()
        assert (ast.cpu().numpy() == was).all() and (aen.cpu().numpy() == wae).all()
        f2, s2, e2 = r.search_all_fused(corpus)
        assert (f2.cpu().numpy() == np.concatenate([[0], np.cumsum(wc)])).all()
        assert (s2.cpu().numpy() == was).all() and (e2.cpu().numpy() == wae).all()
    torch.cuda.synchronize()
    del corpus                                 # rrx_corpus_free with nothing pending
    st, en = r.search_corpus(rr.Corpus(dev, stripe=stripe))        # the regex and the device are as they were
    assert (st.cpu().numpy() == ws).all() and (en.cpu().numpy() == we).all()


def test_three_streams_three_slot_arrays_then_free():
    import synth
    data = synth.corpus("url", 5, 1 << 18)
    want = OracleRegex(U2).match_lines(data)
    corpus = rr.Corpus(torch.from_numpy(data).cuda(), stripe=512)
    r = rr.RRegex(U2)
    r.set_background_order(False)
    assert r.engine_name == "dfa-stride2-table" and corpus.one_launch      # (so: an exchange slot array per stream)
    nw = (corpus.num_lines + 31) // 32
    bits = np.zeros(nw * 32, dtype=np.uint8)
    bits[:len(want)] = want
    want_words = np.packbits(bits, bitorder="little").view(np.uint32)
    got = []
    for k in range(3):
        stream = torch.cuda.Stream()
        out = torch.full((nw,), -1 - k, dtype=torch.int32, device="cuda")      # dirty: the one-launch kernel clears nothing
        stream.wait_stream(torch.cuda.current_stream())
        r.match_corpus_bits(corpus, out=out, stream=stream)
        stream.synchronize()
        got.append(out.cpu().numpy().view(np.uint32))
    assert (got[0] == got[1]).all() and (got[1] == got[2]).all()
    assert (got[0] == want_words).all()
    torch.cuda.synchronize()
    del corpus                                 # three slot arrays go with it, nothing pending
    again = r.match_corpus(rr.Corpus(torch.from_numpy(data).cuda(), stripe=512)).cpu().numpy()
    assert (again == want).all()


def test_automatic_stripe_changes_after_the_first_index():
    """rrx_corpus_create indexes a second time when the stripe the line count asks for is not the one it indexed with.  Below
    256 MiB no text does that (the size-based stripe is 512 bytes there and stripe_for_lines leaves it alone, 1 MiB of 5-byte lines
    included), and from 64 MiB on the stripe is taken from the lines of the first 4 MiB: so 4 MiB of 100-byte lines (the guess from
    them: the size-based 2048 bytes) in front of 254 MiB of 5-byte lines (which want 1024).  The text is periodic, the oracle reads
    one period of each part."""
    rng = np.random.default_rng(3)
    ab = np.frombuffer(b"ab", dtype=np.uint8)
    head = ab[rng.integers(0, 2, size=(512, 100))].copy()
    tail = ab[rng.integers(0, 2, size=(8192, 5))].copy()
    head[:, -1] = tail[:, -1] = 10
    head, tail = head.reshape(-1), tail.reshape(-1)
    data = np.concatenate([np.tile(head, 82), np.tile(tail, 6500)])
    assert 82 * head.size >= (4 << 20) and data.size > (256 << 20)
    o = OracleRegex(ABB)
    want = np.concatenate([np.tile(o.match_lines(head), 82), np.tile(o.match_lines(tail), 6500)])
    size_based = 2048                          # (device.hpp: pick_stripe - more than 2^18 lanes of 1024 bytes)
    corpus = rr.Corpus(torch.from_numpy(data).cuda())
    assert corpus.stripe == 1024 and corpus.stripe != size_based
    assert corpus.num_lines == 82 * 512 + 6500 * 8192 == len(want)
    r = rr.RRegex(ABB)
    r.set_background_order(False)
    got = r.match_corpus(corpus).cpu().numpy()
    assert (got == want).all()
    assert 0 < int(want.sum()) < len(want)
