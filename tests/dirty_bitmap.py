"""A result bitmap written over a DIRTY buffer with guard words behind it: what the GPU tests of the corpus entries share (a word
the kernel does not store, or merges into what it finds, shows at once; so does a word written behind the bitmap)."""
import numpy as np
import torch

FILLS = (-1, 0x55555555, -0x21524111, 0x7FFFFFFF)      # (0xFFFFFFFF, ..., 0xDEADBEEF as int32)


def words_of(want, nwords):
    """The oracle's byte per line as bitmap words, the bits beyond the last line 0."""
    bits = np.zeros(nwords * 32, dtype=np.uint8)
    bits[:len(want)] = want
    return np.packbits(bits, bitorder="little").view(np.uint32)


def run_dirty(call, corpus, want, fill=-1, stream=None, what=""):
    """call(corpus, out=, stream=) over a bitmap pre-filled with `fill`, eight words longer than the corpus needs: every word of
    the bitmap equals the oracle's, the words behind it are untouched."""
    nw = (corpus.num_lines + 31) // 32
    assert len(want) == corpus.num_lines, (what, len(want), corpus.num_lines)
    out = torch.full((nw + 8,), fill, dtype=torch.int32, device="cuda")
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    got = call(corpus, out=out, stream=stream)
    if stream is not None:
        stream.synchronize()
    assert got.numel() == nw
    host = out.cpu().numpy().view(np.uint32)
    bad = np.nonzero(host[:nw] != words_of(want, nw))[0]
    assert bad.size == 0, (what, "word", int(bad[0]), "of", nw, hex(int(host[bad[0]])), hex(int(words_of(want, nw)[bad[0]])))
    assert (host[nw:] == np.uint32(fill & 0xFFFFFFFF)).all(), (what, "words behind the bitmap were written")
