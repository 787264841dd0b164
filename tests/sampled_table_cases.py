"""The case table of the sampled-table match path: the stride-2 kernel with two result bits per line
(match_stripes2_two_bit_kernel = dfa2_body<false, 32, NoPhaseHook, 2>), the split of the wide bitmap (split_two_bit_kernel), and the two
recheck kernels between which the escaped total decides (recheck_lines_kernel, recheck_escaped_kernel), each at the smallest shape that
reaches one of its edges.  Shared by test_sampled_table_lowering.py (no GPU: every case has the property it is named for, its escaping
lines are exactly the ones the table does not decide, the replay of the two-bit form equals the oracle) and test_sampled_table_gpu.py
(the kernels on the same bytes).  Plain Python and numpy; needs neither a GPU nor torch.

    group  stage                      edge
    A1     two-bit stripe kernel      sixteen line ends in a 16-byte slot: the flush after eight bytes (kernels_table.hip: `KB == 2 &&`)
    A2     two-bit stripe kernel      the corpus tail, pair by pair: the threshold 31 - 2 KB, the odd last byte ('\\n', or inside a line)
    A3     two-bit stripe kernel      the line followed past the stripe end; its '\\n' first or second of a pair, an empty line behind it
    A4     two-bit stripe kernel      the wide word two workgroups share, with 0, 2 and 30 bits of the first one
    A5     two-bit stripe kernel      more wide words per workgroup than the LDS window holds
    B1     split                      bitmaps of 1, 255, 256, 257 words, the last one with 1, 31 and 32 lines
    B2     split                      2048, 2049 and 8192 escaped lines in one workgroup's turn: the flush inside the turn
    B3     split                      a second turn of the grid (more than 2048 x 256 words)
    C      list / walk hand-over      escaped totals of cap - 1, cap, cap + 1, cap = the floor and cap = words / 2
    D      recheck_lines_kernel       where the listed line's preceding '\\n' lies: in its 64 bytes, its 16 bytes, its stripe, the data
    E      recheck_escaped_kernel     the same placements with more escaped lines than the list holds; stripes without a line start"""
import random
from collections import namedtuple

import numpy as np

from nfa_width_cases import SAMPLED_LIST_FLOOR, SAMPLED_RETIRE_PERCENT, sampled_list_capacity

# The pattern: nullable (an empty line is accepted: a '\n' run is a run of ACCEPTED lines), on the NFA lane engine under AUTO with two
# words per set, and with the SAMPLE below its table decides lines of 0 ... 4 bytes of a-d with both verdicts and ESCAPES on an x/y
# line from twelve x on; such a line is accepted exactly when an x stands 41 bytes from its end.  (test_sampled_table_lowering.py pins
# all of this; a change of the table build that moves it wants another pattern with the same four properties.)
PATTERN = "([a-c]?[a-c]?[a-c]?)|(x|y)*x(x|y){40}"
TAIL = 40                                 # the pattern's {40}

K_ROUND = 128                             # device.hpp: kRound - bytes a lane steps between two loads
K_THREADS = 1024                          # device.hpp: kThreads (RRX_THREADS) - stripes per workgroup of the stripe kernel
MIN_STRIPE, MAX_STRIPE = 512, 16384       # device.hpp: kMinStripe, kMaxStripe
WINDOW_WORDS_MAX = 46 * 1024 // 4         # device.hpp: kDfa2RegionBytes = 46 KiB: no table leaves a result window of more words
SPLIT_LOCAL, SPLIT_FLUSH_AT = 4096, 2048  # kernels_table.hip, split_two_bit_kernel: kLocal, kFlushAt = kLocal - 256 * 8
SPLIT_BLOCK_WORDS = 256                   # kernels_table.hip, split_two_bit_kernel: __launch_bounds__(256), a bitmap word (32 lines) per lane
SPLIT_GRID_MAX = 2048                     # kernels_table.hip, split_two_bit: `if (blocks > 2048) blocks = 2048`
SPLIT_TURN_LINES = SPLIT_GRID_MAX * SPLIT_BLOCK_WORDS * 32
BLOCK_LINES = SPLIT_BLOCK_WORDS * 32      # the lines of one split workgroup's turn
RETIRE_PERCENT = SAMPLED_RETIRE_PERCENT   # sampled.hpp: kRetireEscapePercent (defined once: nfa_width_cases.py)
LIST_FLOOR = SAMPLED_LIST_FLOOR           # corpus.cpp, match_corpus_sampled: cap = max(words / 2, 1024) (defined once: nfa_width_cases.py)

ER = b"x" * 12                            # the shortest escaping line: rejected
EA = b"x" + b"y" * TAIL                   # the shortest accepted one: 41 bytes
# A NUL is of byte class 0, and class 0 leads from every state of the table, ESCAPE included, to the dead state: a line that holds one is
# REJECTED BY THE TABLE wherever the NUL stands, and never reaches the recheck kernels (the lowering test pins both lines as decided)
NUL_INSIDE = b"x" * 20 + b"\x00" + b"x" * (TAIL + 1)      # in the ESCAPE state when the NUL comes
NUL_IN_FRONT = b"\x00" + b"x" * (TAIL + 1)
ER_CLASS1 = b"x" * 12 + b"a"              # ESCAPE loops on the a-c class too: escaping, rejected
DECIDED = (b"", b"a", b"ab", b"abc", b"abcd", b"d", b"x", b"xyx", b"y" * 45)      # the table decides these: 4 accepted, 5 rejected


def sample():
    """the text the table is learnt from: 2000 lines"""
    rng = random.Random(3)
    out = []
    for _ in range(2000):
        k = rng.random()
        if k < 0.7:
            out.append("".join(rng.choice("abc") for _ in range(rng.randint(0, 3))))
        elif k < 0.8:
            out.append("d" * rng.randint(1, 3))
        elif k < 0.9:
            out.append("".join(rng.choice("abc") for _ in range(4)))
        else:
            out.append(rng.choice(("x", "y", "xy", "yx")))
    return ("\n".join(out) + "\n").encode()


def esc(length, accept):
    """an escaping line of `length` >= 53 bytes: twelve x and more in front, the byte 41 from the end decides"""
    assert length >= 12 + TAIL + 1
    return b"x" * (length - TAIL - 1) + (b"x" if accept else b"y") + b"x" * TAIL


def esc_short(accept):
    return EA if accept else ER


Built = namedtuple("Built", "data vocab idx escaping final_newline notes")
# data: numpy uint8, read-only; vocab: the distinct lines; idx: vocabulary index per line; escaping: indices of the lines built to
# escape (sorted); notes: what the lowering test needs to find the case's edge (byte offsets, line numbers)


class _Lines:
    """a corpus line by line, with the byte offset kept"""

    def __init__(self):
        self.lines, self.off, self.escaping = [], 0, []

    def add(self, line, escaping=False):
        if escaping:
            self.escaping.append(len(self.lines))
        self.lines.append(line)
        self.off += len(line) + 1
        return len(self.lines) - 1

    def add_esc(self, line):
        return self.add(line, True)

    def pad_to(self, target):
        """rejected filler lines of d (the table decides them) up to byte offset `target`"""
        gap = target - self.off
        assert gap >= 0, (target, self.off)
        while gap > 64:
            self.add(b"d" * 47)
            gap -= 48
        if gap:
            self.add(b"d" * (gap - 1))

    def pad_mod(self, residue, mod):
        self.pad_to(self.off + (residue - self.off) % mod)

    def bulk(self, n, rng, vocab=(b"a", b"d")):
        for _ in range(n):
            self.add(rng.choice(vocab))

    def built(self, final_newline=True, **notes):
        index, vocab = {}, []
        idx = np.empty(len(self.lines), dtype=np.int32)
        for i, t in enumerate(self.lines):
            k = index.get(t)
            if k is None:
                k = index[t] = len(vocab)
                vocab.append(t)
            idx[i] = k
        data = np.frombuffer(b"\n".join(self.lines) + (b"\n" if final_newline else b""), dtype=np.uint8)
        assert final_newline or self.lines[-1], "an empty last line without its newline is no line"
        return Built(data, vocab, idx, np.array(self.escaping, dtype=np.int64), final_newline, notes)


def _assemble(vocab, idx):
    """the corpus of the lines vocab[idx], every line with its '\\n', in numpy (the one large case)"""
    vlen = np.array([len(v) for v in vocab], dtype=np.int64)
    lens = vlen[idx] + 1
    ends = np.cumsum(lens)
    data = np.full(int(ends[-1]), 10, dtype=np.uint8)
    starts = ends - lens
    for k, v in enumerate(vocab):
        if v:
            at = starts[idx == k]
            data[(at[:, None] + np.arange(len(v))[None, :]).reshape(-1)] = np.tile(np.frombuffer(v, dtype=np.uint8), len(at))
    return data


# ---- A: the two-bit stripe kernel
def _a1():
    """runs of 70 ... 85 '\\n' and of forty a\\n / d\\n whose first byte lies at every residue mod 16, a line of known verdict in front of
    and behind each (escaping ones among them); the corpus is whole rounds of every stripe up to 4096"""
    rng = random.Random(11)
    b = _Lines()
    runs = []
    for residue in range(16):
        for kind in range(4):
            front = (esc_short(kind % 2 == 0), b"abcd", b"abc", ER)[(residue + kind) % 4]
            b.pad_mod((residue - len(front) - 1) % 16, 16)
            b.add(front, front in (ER, EA))
            assert b.off % 16 == residue
            runs.append((b.off, kind))
            if kind == 0:
                for _ in range(70 + residue):
                    b.add(b"")
            elif kind == 1:
                for _ in range(40):
                    b.add(b"a")
            elif kind == 2:
                for _ in range(40):
                    b.add(b"d")
            else:
                for k in range(24):                          # '\n' '\n' a '\n': three line ends in four bytes
                    b.add(b"")
                    b.add(b"")
                    b.add(rng.choice((b"a", b"d")))
            behind = (EA, b"ab", ER, b"abcd")[(residue + kind) % 4]
            b.add(behind, behind in (ER, EA))
    b.bulk(3000, rng)                                        # (the escaping lines stay below 5 % of the lines)
    b.pad_to((b.off + 4096 + 4095) // 4096 * 4096)
    return b.built(runs=runs)


A2_PAIRS = (1, 8, 14, 31, 62, 63)         # '\n' pairs in the partial round: 2 ... 126 bytes with the odd byte below (63 pairs: without one)


def _a2(layout, pairs, end):
    """The last stripe (at 512 and at 4096: it begins at byte 8192) is one whole round and a partial round of `pairs` '\\n' pairs, then
    nothing (end = "even"), one more '\\n' ("nl": the odd last byte is a '\\n') or one letter ("open": the odd last byte lies in a last line
    without its newline).  layout "inside": the round lies inside an escaping line that began in the stripe before and ends with the
    partial round's first byte - the lane holds no result when the pairs begin; "fresh": the round holds two lines, one of them escaping."""
    rng = random.Random(pairs * 7 + len(end))
    b = _Lines()
    b.add_esc(ER)
    b.add_esc(EA)
    b.bulk(1500, rng)
    cut, tail = 8192, 2 * pairs
    if layout == "inside":
        b.pad_to(cut - 100)
        b.add_esc(esc(100 + K_ROUND, pairs % 2 == 0))        # its '\n' is the partial round's first byte
        tail -= 1
    else:
        b.pad_to(cut)
        b.add_esc(EA)
        b.add(b"d" * (K_ROUND - len(EA) - 2))
    assert b.off == cut + K_ROUND + (1 if layout == "inside" else 0)
    for _ in range(tail + (1 if end == "nl" else 0)):
        b.add(b"")
    if end == "open":
        b.add(b"a" if pairs % 2 == 0 else b"d")
    return b.built(final_newline=end != "open", cut=cut, tail=2 * pairs + (0 if end == "even" else 1))


A3_ENDS = (0, 1, 14, 15, 126, 127, 128, 129, 200, 201)    # the '\n' of the straddling line, in bytes behind the stripe end: both bytes of a
                                                          # pair, inside and behind the 128 bytes the lane has requested in advance


def _a3():
    """escaping lines that begin 60 bytes in front of a multiple of 4096 (a stripe end at every stripe) and end e bytes behind it, or
    512 + e, 1024 + e, 8192 + e: the line spans one stripe end, two, three (stripes wholly inside it), and three at stripe 4096; behind
    each an empty line (the pair of its '\\n' then holds two line ends where e is even), or a line of one byte"""
    b = _Lines()
    placed = []
    for extra in (0, 512, 1024, 8192):
        for i, e in enumerate(A3_ENDS if extra == 0 else (0, 1, 127, 128)):
            for j, behind in enumerate((b"", b"a", b"d")):
                boundary = (b.off + 60 + 4095) // 4096 * 4096
                b.pad_to(boundary - 60)
                at = b.add_esc(esc(60 + extra + e, (i // 2 + j) % 2 == 0))      # (both verdicts at both parities of e, for every `behind`)
                assert b.off - 1 == boundary + extra + e
                b.add(behind)
                placed.append((at, boundary, extra, e, behind))
    b.pad_to((b.off + 4095) // 4096 * 4096 + 300)
    return b.built(placed=placed)


A4_CUT = K_THREADS * MIN_STRIPE           # the second workgroup's first byte at stripe 512


def _a4(lines_mod_16, fresh):
    """Two workgroups at stripe 512 with `lines_mod_16` (mod 16) line ends in front of the second one's first stripe, which begins a
    line (fresh: an escaping line ends with the byte in front of it) or lies inside an escaping line."""
    rng = random.Random(40 + lines_mod_16 * 2 + fresh)
    vocab = (b"", b"a", b"d", b"abc", b"abcd", b"d" * 23, b"d" * 47, b"y" * 30, b"ab")
    b = _Lines()
    while b.off < A4_CUT - 700:
        if len(b.lines) % 400 == 399:
            b.add_esc(esc_short(len(b.lines) % 800 == 399))
        else:
            b.add(rng.choice(vocab))
    for _ in range((lines_mod_16 - len(b.lines) - (1 if fresh else 0)) % 16):
        b.add(b"a")
    gap = A4_CUT - b.off
    assert gap > 64
    straddler = b.add_esc(esc(gap - 1 if fresh else gap + 37, lines_mod_16 != 1))
    for k in range(600):
        if k % 100 == 50:
            b.add_esc(esc_short(k % 200 == 50))
        else:
            b.add(rng.choice(vocab))
    return b.built(straddler=straddler, lines_mod_16=lines_mod_16, fresh=fresh)


A5_PLANTED = (5, 1000, 190000, 200001, 250002, 262000, 262600, 300000, 455000, 460001, 500002, 523000)
_A5_SET = frozenset(A5_PLANTED)


def _a5():
    """1 MiB of 2-byte lines: at stripe 512 a workgroup's 512 KiB hold 262144 lines, 16384 wide words, and no window holds more than
    11776; escaping lines in front of and beyond the window of both workgroups"""
    rng = random.Random(50)
    b = _Lines()
    for i in range(524288 - 400):
        if i in _A5_SET:
            b.add_esc(esc_short(A5_PLANTED.index(i) % 2 == 0))
        else:
            b.add(b"a" if rng.random() < 0.5 else b"d")
    return b.built()


# ---- B: the split
def _b1(words, last):
    """a bitmap of `words` words whose last word holds `last` lines: 1-byte lines and two escaping ones (a bitmap of one word: at most
    one - two among 32 lines are more than the 5 % every case stays within; none in a corpus of one line)"""
    rng = random.Random(words * 32 + last)
    n = 32 * (words - 1) + last
    b = _Lines()
    planted = {} if n < 20 else {n // 2: words % 2 == 0} if n < 64 else {n // 3: True, n - 2: False}
    for i in range(n):
        if i in planted:
            b.add_esc(esc_short(planted[i]))
        else:
            b.add(b"a" if rng.random() < 0.5 else b"d")
    return b.built()


B2_LINES = 21 * BLOCK_LINES               # 8192 escaping lines are 4.8 % of them; 5376 bitmap words: cap = 2688
B2_BLOCK = 3                              # the block of lines 24576 ... 32767: one split workgroup's turn


def _b2(escaping):
    """1-byte lines, and in the one block of 8192 lines that split workgroup 3 takes in its turn `escaping` escaping lines: 2048 (eight
    per lane: the local buffer holds kFlushAt entries when the turn ends, no flush inside it), 2049 (one flush inside the turn), 8192"""
    rng = random.Random(escaping)
    lo = B2_BLOCK * BLOCK_LINES
    if escaping == BLOCK_LINES:
        chosen = set(range(lo, lo + BLOCK_LINES))
    else:
        chosen = set(range(lo, lo + BLOCK_LINES, 4))
        if escaping == 2049:
            chosen.add(lo + 4097)
    assert len(chosen) == escaping
    b = _Lines()
    for i in range(B2_LINES):
        if i in chosen:
            b.add_esc(esc_short(i % 3 == 0))
        else:
            b.add(b"a" if rng.random() < 0.5 else b"d")
    return b.built(block=(lo, lo + BLOCK_LINES))


B3_LINES = SPLIT_TURN_LINES + 3 * BLOCK_LINES + 17
B3_PLANTED = (0, 31, 32, 8191, 5_000_000, SPLIT_TURN_LINES - BLOCK_LINES, SPLIT_TURN_LINES - 33, SPLIT_TURN_LINES - 32, SPLIT_TURN_LINES - 1,
              SPLIT_TURN_LINES, SPLIT_TURN_LINES + 1, SPLIT_TURN_LINES + 31, SPLIT_TURN_LINES + 32, SPLIT_TURN_LINES + BLOCK_LINES - 1,
              SPLIT_TURN_LINES + BLOCK_LINES, SPLIT_TURN_LINES + 2 * BLOCK_LINES + 5, B3_LINES - 18, B3_LINES - 1)


def _b3():
    """more lines than one turn of the split's grid takes (2048 x 256 words of 32): empty and 1-byte lines, with escaping lines
    on both sides of the turn boundary, in the first and in the last word.  THE one large case (27 MiB)."""
    rng = np.random.default_rng(60)
    vocab = [b"", b"a", b"d", ER, EA]
    idx = rng.integers(0, 3, size=B3_LINES).astype(np.int32)
    planted = np.array(B3_PLANTED, dtype=np.int64)
    idx[planted] = 3 + (np.arange(len(planted)) % 2)
    data = _assemble(vocab, idx)
    return Built(data, vocab, idx, planted, True, {})


# ---- C: the hand-over between the list and the walk
def _c(nlines, total):
    """1-byte lines with `total` escaping ones spread evenly"""
    rng = random.Random(total)
    chosen = {int(k * nlines / total) for k in range(total)}
    assert len(chosen) == total
    b = _Lines()
    for i in range(nlines):
        if i in chosen:
            b.add_esc(esc_short(i % 3 == 0))
        else:
            b.add(b"a" if rng.random() < 0.5 else b"d")
    return b.built()


# ---- D, E: where a line that escapes begins
D_RESIDUES = (0, 15, 16, 47, 63)          # offset mod 64 of the '\n' in front of a listed line


def _placements(b, rng):
    """-> {name: line index}: escaping lines at the places the two recheck kernels find a line start in different ways"""
    at = {}
    at["line 0"] = b.add_esc(EA)
    b.bulk(40, rng)
    for k, residue in enumerate(D_RESIDUES):                  # the preceding '\n' at these offsets mod 64
        b.pad_mod((residue + 1) % 64, 64)
        at["mod 64 = %d" % residue] = b.add_esc(esc_short(k % 2 == 1))
        b.bulk(7, rng)
    for stripe in (512, 4096):                               # ... as the last byte of a stripe: the line is the stripe's first
        b.pad_mod(0, stripe)
        at["behind stripe %d" % stripe] = b.add_esc(esc_short(stripe == 512))
        b.bulk(5, rng)
    for k, nth in enumerate((1, 8, 16)):                     # ... as the nth '\n' of its sixteen bytes, behind a dense region
        b.pad_mod(0, 64)
        for _ in range(64 + nth):
            b.add(b"")
        assert b.off % 16 == nth % 16
        at["newline %d of its 16 bytes" % nth] = b.add_esc(esc_short(k % 2 == 0))
        b.bulk(9, rng)
    at["NUL inside"] = b.add(NUL_INSIDE)                     # (the table decides both: see NUL_INSIDE)
    b.bulk(3, rng)
    at["NUL in front"] = b.add(NUL_IN_FRONT)
    b.bulk(3, rng)
    at["a behind the tail"] = b.add_esc(ER_CLASS1)
    b.bulk(30, rng)
    return at


def _ends(b, at, final_newline):
    """the last two lines: one that begins less than 64 bytes in front of the end of the data, one less than 16"""
    at["less than 64 from the end"] = b.add_esc(EA)
    at["less than 16 from the end"] = b.add_esc(ER)
    return b.built(final_newline=final_newline, at=at)


def _d(final_newline):
    rng = random.Random(70 + final_newline)
    b = _Lines()
    at = _placements(b, rng)
    b.bulk(400, rng)
    return _ends(b, at, final_newline)


E_EXTRA = LIST_FLOOR + 80                 # escaping lines of the bulk: with the placed ones, more than the list holds


def _region(b, at, unit):
    """three stripes of `unit` bytes: one whose FIRST line is its only escaping one, one whose LAST line is - a line that goes on through
    the whole of the next stripe (no line starts there) and ends in the one after"""
    b.pad_mod(0, unit)
    lo = b.off
    at["first of stripe %d" % unit] = b.add_esc(ER)
    b.pad_to(lo + unit)
    b.add(b"d" * 20)
    b.pad_to(lo + 2 * unit - 30)
    at["last of stripe %d" % unit] = b.add_esc(esc(30 + unit + 70, True))
    at["no line starts %d" % unit] = lo + 2 * unit                        # (a byte offset: the stripe that begins there)
    b.pad_to(lo + 4 * unit)


def _e(final_newline):
    rng = random.Random(80 + final_newline)
    b = _Lines()
    at = _placements(b, rng)
    for unit in (512, 4096):
        _region(b, at, unit)
    for k in range(E_EXTRA):                                 # 23 lines between two escaping ones: 4.2 %
        b.add_esc(esc_short(k % 2 == 0))
        b.bulk(23, rng, (b"a", b"d", b"", b"abcd", b"d" * 30))
    return _ends(b, at, final_newline)


Case = namedtuple("Case", "id group build stripes path both_verdicts")
# stripes: the stripes the GPU test runs the case at (0: the automatic one); path: "list" or "walk", by the escaped total and the cap;
# both_verdicts: the case holds an accepted and a rejected escaping line (all but the bitmaps of one word)


def _table():
    out = [Case("A1-dense", "A1", _a1, (512, 4096), "list", True)]
    for layout in ("inside", "fresh"):
        for pairs in A2_PAIRS:
            for end in ("even", "nl", "open") if pairs < 63 else ("even",):
                out.append(Case("A2-%s-%d-%s" % (layout, pairs, end), "A2", lambda a=layout, p=pairs, e=end: _a2(a, p, e), (512, 4096), "list", True))
    out.append(Case("A3-follow", "A3", _a3, (512, 4096), "list", True))
    for k in (0, 1, 15):
        for fresh in (True, False):
            out.append(Case("A4-%d-%s" % (k, "fresh" if fresh else "inside"), "A4", lambda k=k, f=fresh: _a4(k, f), (512,), "list", True))
    out.append(Case("A5-window", "A5", _a5, (512, 4096), "list", True))
    for words in (1, 255, 256, 257):
        for last in (1, 31, 32):
            out.append(Case("B1-%d-%d" % (words, last % 32), "B1", lambda w=words, m=last: _b1(w, m), (512,), "list", words > 1))
    out.append(Case("B2-2048", "B2", lambda: _b2(2048), (512, 4096), "list", True))
    out.append(Case("B2-2049", "B2", lambda: _b2(2049), (512, 4096), "list", True))
    out.append(Case("B2-8192", "B2", lambda: _b2(BLOCK_LINES), (512, 4096), "walk", True))
    out.append(Case("B3-second-turn", "B3", _b3, (0,), "list", True))
    for nlines, cap in ((32768, 1024), (131072, 2048)):
        for total in (cap - 1, cap, cap + 1):
            out.append(Case("C-%d-%d" % (cap, total), "C", lambda n=nlines, t=total: _c(n, t), (512,), "list" if total <= cap else "walk", True))
    for final_newline in (True, False):
        tag = "newline" if final_newline else "open"
        out.append(Case("D-" + tag, "D", lambda f=final_newline: _d(f), (512, 4096, 0), "list", True))
        out.append(Case("E-" + tag, "E", lambda f=final_newline: _e(f), (512, 4096, 0), "walk", True))
    return out


CASES = _table()
GROUPS = ("A1", "A2", "A3", "A4", "A5", "B1", "B2", "B3", "C", "D", "E")
REPLAY_LIMIT = 1 << 20                    # cases up to this size: the replay of the two-bit form and the oracle over the whole text
_built = {}


def built(case):
    """the case's corpus, the same object on every call"""
    if case.id not in _built:
        b = case.build()
        b.data.setflags(write=False)
        _built[case.id] = b
    return _built[case.id]


def of_group(group):
    return [c for c in CASES if c.group == group]


def list_capacity(nlines):
    return sampled_list_capacity(nlines)


def expected(case, oracle):
    """the oracle's verdict per line (numpy uint8), taken per distinct line"""
    b = built(case)
    return np.array([1 if oracle.accepts(v) else 0 for v in b.vocab], dtype=np.uint8)[b.idx]


def line_starts(data):
    """byte offset of every line's first byte (a last line without its newline included)"""
    nl = np.nonzero(np.asarray(data) == 10)[0]
    starts = np.concatenate([[0], nl + 1])
    return starts[:-1] if len(data) and data[-1] == 10 else starts
