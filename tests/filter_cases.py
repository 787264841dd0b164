"""What the filter tests share (test_filter_lowering.py, test_filter_gpu.py): the RULE of rrx_bitmap_rank / rrx_filter_* in Python,
built with numpy on the host, and the case table - bitmap sizes, item counts and the texts of the corpus cases, each text built so
that it has the geometry its name claims (asserted here, at import: a stripe is 512 bytes in every corpus case but the last)."""
import numpy as np

STRIPE = 512
ROUND = 128                                     # device.hpp: kRound, the bytes of one TextRound
SCAN_CHUNK = 4096                               # kernels_index.hip: kScanChunk, the counts one workgroup of the scan takes
MAX_LANES = 512 * 1024                          # device.hpp: kFilterMaxBlocks workgroups of 1024 lanes, then the items grid strides

# rank: the bits of a bitmap around a word, around the 2048 bits of a wave of the popcount kernel, word counts around one chunk of
# the scan, and one bitmap of more than 1024 chunks (the second level of the scan then sums more than one chunk per lane)
RANK_NBITS = (0, 1, 31, 32, 33, 2047, 2048, 2049)
RANK_NWORDS = (SCAN_CHUNK - 1, SCAN_CHUNK, SCAN_CHUNK + 1)
RANK_LARGE_NWORDS = 1024 * SCAN_CHUNK + SCAN_CHUNK + 5
ITEM_COUNTS = (1, 31, 32, 33, 1023, 1025, MAX_LANES + 1)
SELECTIONS = ("none", "all", "first", "last", "alternating", "random")


# ---------------------------------------------------------------------------------------------------------------- the rule
def selected_rows(bits, n, invert):
    """The rule's selection: row i < n is selected iff bit i & 31 of word i >> 5 is 1 (invert: 0).  Bits beyond n: never."""
    words = np.asarray(bits).view(np.uint32)
    flat = np.unpackbits(words[:(n + 31) // 32].view(np.uint8), bitorder="little")[:n].astype(bool)
    return np.nonzero(~flat if invert else flat)[0].astype(np.int64)


_POPCOUNT = np.array([bin(v).count("1") for v in range(256)], dtype=np.int64)


def rank_rule(bits, n, invert):
    """d_rank[0 .. nwords]: the selected rows in front of every word, and all of them (word by word: bitmaps of 16 MiB too)."""
    nw = (n + 31) // 32
    w = np.asarray(bits).view(np.uint32)[:nw].copy()
    if invert:
        w = ~w
    if n % 32:
        w[-1] &= np.uint32((1 << (n % 32)) - 1)
    per_word = _POPCOUNT[w.view(np.uint8)].reshape(nw, 4).sum(axis=1)
    return np.concatenate([[0], np.cumsum(per_word)]).astype(np.uint64)


def lines_of(text):
    """[(line without its '\\n', has a '\\n' in the text)]: a final fragment without '\\n' is a line, an empty text has none."""
    text = bytes(text)
    parts = text.split(b"\n")
    tail = parts.pop()
    return [(p, True) for p in parts] + ([(tail, False)] if tail else [])


def filter_rule(items_or_lines, bits, invert=False, keep_newline=False):
    """The rule.  items_or_lines: a list of items (bytes, the separator already trimmed) or a '\\n'-text (bytes: its lines).
    -> (rows int64, offsets int64 [len(rows) + 1], bytes): the selected rows' numbers, the new column's offsets and its bytes;
    a line keeps its '\\n' iff keep_newline and the text has it."""
    if isinstance(items_or_lines, (bytes, bytearray)):
        rows_in = [ln + (b"\n" if keep_newline and nl else b"") for ln, nl in lines_of(items_or_lines)]
    else:
        rows_in = [bytes(x) for x in items_or_lines]
    rows = selected_rows(bits, len(rows_in), invert)
    picked = [rows_in[i] for i in rows]
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in picked])]).astype(np.int64)
    return rows, offsets, b"".join(picked)


def sources_rule(items_or_lines, bits, invert=False, first=0, trim=0):
    """d_piece_src of the selected rows: the absolute offset of each one's first byte (items: with `trim` separator bytes behind
    every item and the first item at `first`)."""
    if isinstance(items_or_lines, (bytes, bytearray)):
        lens = [len(ln) + (1 if nl else 0) for ln, nl in lines_of(items_or_lines)]
    else:
        lens = [len(x) + trim for x in items_or_lines]
    starts = first + np.concatenate([[0], np.cumsum(lens)])[:-1].astype(np.int64) if lens else np.zeros(0, dtype=np.int64)
    return starts[selected_rows(bits, len(lens), invert)]


def pack_bits(flags, rng):
    """A bool per row -> bitmap words, the spare bits of the last word set to garbage."""
    n = len(flags)
    nw = (n + 31) // 32
    full = rng.integers(0, 2, size=nw * 32).astype(np.uint8)
    if n % 32:
        full[n + 1:] |= 1                                          # (not only random garbage: most spare bits are 1)
    full[:n] = np.asarray(flags, dtype=np.uint8)
    return np.packbits(full, bitorder="little").view(np.uint32).copy()


def selection(kind, n, rng):
    f = np.zeros(n, dtype=bool)
    if kind == "all":
        f[:] = True
    elif kind == "first":
        f[:1] = True
    elif kind == "last":
        f[-1:] = True
    elif kind == "alternating":
        f[::2] = True
    elif kind == "random":
        f = rng.integers(0, 3, size=n) == 0
    else:
        assert kind == "none"
    return f


# ---------------------------------------------------------------------------------------------------------------- corpus texts
def text_of(lengths, final_newline=True):
    """Lines of the given lengths, line k filled with a letter of its own and its last byte a digit; every line but - without
    final_newline - the last ends in '\\n'."""
    out = []
    for k, n in enumerate(lengths):
        body = bytes([97 + k % 26]) * n
        if n:
            body = body[:-1] + bytes([48 + k % 10])
        out.append(body)
    return b"\n".join(out) + (b"\n" if final_newline else b"")


def line_starts(text):
    lens = [len(ln) + (1 if nl else 0) for ln, nl in lines_of(text)]
    return np.concatenate([[0], np.cumsum(lens)])[:-1].astype(np.int64)


def stripe_ends_spanned(text, k):
    """The stripe ends that line k crosses: its first byte lies in one stripe, its '\\n' (or its last byte) that many further on."""
    ln, nl = lines_of(text)[k]
    a = int(line_starts(text)[k])
    b = a + len(ln) - (0 if nl else 1)
    return b // STRIPE - a // STRIPE


def stripes_without_a_line_start(text):
    starts = set(int(s) // STRIPE for s in line_starts(text))
    return [g for g in range((len(text) + STRIPE - 1) // STRIPE) if g not in starts]


def _spans():
    t = text_of([99, 600, 1100, 1700, 50, 7])
    assert [stripe_ends_spanned(t, k) for k in (1, 2, 3)] == [1, 2, 3] and stripes_without_a_line_start(t) == [2, 4, 5]
    return t


def _stripe_edges():
    # line 1 starts on the last byte of stripe 0 and its '\n' is the first byte of stripe 1; the '\n' of line 2 is the last byte of
    # stripe 1; line 4 starts on the last byte of stripe 2 and runs into stripe 3
    t = text_of([510, 1, 510, 510, 300, 20])
    s = line_starts(t)
    assert s[1] == STRIPE - 1 and t[STRIPE] == 10 and t[2 * STRIPE - 1] == 10 and s[4] == 3 * STRIPE - 1 and stripe_ends_spanned(t, 4) == 1
    return t


def _empty_runs():
    return b"\n" * 40 + b"x\n" + b"\n" * 700 + b"yy\n" + b"\n" * 33 + b"z"


def _tail_behind_line_start(tail, final_newline):
    """A text of two stripes and a bit: its last line starts `tail` bytes (its '\\n' included, if any) in front of the end of the data."""
    body = tail - (1 if final_newline else 0)
    t = text_of([300, 400, 2 * STRIPE + 40 - 702 - tail - 1, body], final_newline)
    assert len(t) == 2 * STRIPE + 40 and len(t) - int(line_starts(t)[-1]) == tail
    return t


def _sparse_waves():
    """Three waves of stripes (64 stripes of 512 bytes each) of 37-byte lines: the selection names no line that starts in wave 0,
    exactly one that starts in wave 1 and every third one of wave 2."""
    t = text_of([36] * (3 * 64 * STRIPE // 37))
    s = line_starts(t)
    wave = s // (64 * STRIPE)
    f = np.zeros(len(s), dtype=bool)
    f[np.nonzero(wave == 1)[0][200]] = True
    f[np.nonzero(wave == 2)[0][::3]] = True
    assert f[wave == 0].sum() == 0 and f[wave == 1].sum() == 1 and f[wave == 2].sum() > 64
    return t, f


def _random_text(rng, nbytes, newline_every):
    a = rng.integers(97, 123, size=nbytes).astype(np.uint8)
    a[rng.integers(0, newline_every, size=nbytes) == 0] = 10
    return a.tobytes()


def corpus_cases():
    """[(name, text, extra selections: [(name, bool per line)])] - every case also runs the SELECTIONS."""
    rng = np.random.default_rng(20261021)
    spans = _spans()
    sparse_text, sparse_sel = _sparse_waves()
    cases = [
        ("a selected line spans one, two and three stripe ends; stripes 2, 4, 5 start no line", spans,
         [("the spanning lines", np.array([0, 1, 1, 1, 0, 0], bool)), ("only the last spanning line", np.array([0, 0, 0, 1, 0, 0], bool))]),
        ("lines start on the last byte of a stripe; a newline is the first and the last byte of a stripe", _stripe_edges(),
         [("the lines at the edges", np.array([0, 1, 1, 0, 1, 0], bool))]),
        ("runs of empty lines", _empty_runs(), []),
        ("only newlines, three stripes", b"\n" * (3 * STRIPE - 11), []),
        ("one newline", b"\n", []),
        ("one line without a newline", b"abc", []),
        ("a final fragment without a newline", b"abc\ndef\n\nghi", [("the fragment", np.array([0, 0, 0, 1], bool)), ("all but the fragment", np.array([1, 1, 1, 0], bool))]),
        ("a final fragment without a newline that starts in the last stripe", text_of([500, 600, 9], False), [("the fragment", np.array([0, 0, 1], bool))]),
        ("a wave with one selected line, a wave with none", sparse_text, [("sparse", sparse_sel)]),
    ]
    for tail in (1, 9, 15, 16, 17, 100, ROUND - 1, ROUND, ROUND + 1):
        for final_newline in (True, False):
            cases.append(("the data ends %d bytes behind the last line start, final newline %s" % (tail, final_newline),
                          _tail_behind_line_start(tail, final_newline), [("the last line", np.array([0, 0, 0, 1], bool))]))
    cases.append(("random text, short lines", _random_text(rng, 40 * STRIPE + 77, 12), []))
    cases.append(("random text, lines of about two stripes", _random_text(rng, 40 * STRIPE + 3, 1000), []))
    return cases


def automatic_stripe_text():
    return _random_text(np.random.default_rng(7), 300_000, 30) + b"the end"


# ---------------------------------------------------------------------------------------------------------------- one-call data
ONE_CALL_PATTERNS = (r"[0-9]+", r"error|warn|fatal")
ONE_CALL_LINES = [b"GET /index.html 200", b"", b"error: disk 7 full", b"all quiet", b"warn", b"fatal flaw", b"w a r n", b"12", b"no digits here",
                  b"x" * 70 + b"9", b"error", b"y" * 300]
