"""Corpora for the stripe-wise search kernel (kernels_search.hip) with an expectation that replays no device table.  Host only.

CELLS.  A line is a sequence of parts: cells of at most 24 bytes over the pattern's alphabet, and inert bytes between them - runs of
a separator that no match of the pattern can contain or span (' ' for every pattern of SPECS), NUL and bytes >= 0x80.  What a line
must give follows from the oracle's brute force on each cell alone (OracleRegex.search_all), shifted by the cell's offset: the first
match is that of the first cell that has one, all matches are the cells' matches in order.  tests/test_search_corpus_cases.py proves
the separator argument per pattern (the composed answer against the replay of the search tables on the whole line) and that every
case puts its features where its name says.  A part whose matches are known by construction (one long needle, a run of two-byte
matches) carries them, confirmed by OracleRegex.accepts.  Patterns that accept the empty string have a closed form.

Every builder takes target offsets: `CaseBuilder.place` pads with short lines until the named byte of the next line - its first
byte, its '\\n', the last or the first byte of a match - has the wanted residue of a lane (256 bytes), an event word (16), a pair (2),
a walk's word (4) or a chunk (16384), and `finish` asserts that every requested placement is there."""
import random
from collections import namedtuple

import numpy as np

from patterns import EMAIL
from pyoracle import OracleRegex

PAIR, WALK, WORD, LANE, CHUNK = 2, 4, 16, 256, 16384    # kernels_search.hip: byte pair, text word of a walk, event word, kSearchS, kSearchChunk
MAX_CELL = 24
NUMBER, KEYWORD, LONG = "[0-9]+\\.[0-9]+", "k(1|10|100)", "b(a|c)*d"
GLOBAL_FORM = "[ab]*a[ab]{11}x"                          # its product table does not fit the LDS: the kernel's global form
BOUNDED = "(aaa)*b|ca"                                   # a walk back that must stop at the end of the match before: "caaab" is "ca" + "b",
                                                         # and "aaab", which starts inside "ca", is accepted too
_H = b"a" + b"bababbababa" + b"x"                        # GLOBAL_FORM: 'a', eleven of [ab], 'x'

Spec = namedtuple("Spec", "sep lead inner miss sized")
# lead: cells whose first match starts at their first byte (at a line start: a hit that knows its start); inner: it starts behind
# junk (a walk back); miss: no match; sized: four inner cells whose match lengths are 0, 1, 2, 3 mod 4
SPECS = {
    "ab+c": Spec(b" ", [b"abc", b"abbbc", b"abcabbc"], [b"bbabc", b"cbabbbbc", b"babcbbabbc"], [b"ab", b"bbc", b"acb", b"bbbbbbbc"],
                 [b"bbabbc", b"bbabbbc", b"bbabbbbc", b"bbabc"]),
    NUMBER: Spec(b" ", [b"1.5", b"12.25"], [b".7.5", b"..12.3"], [b"12.", b".5", b"7"], None),
    KEYWORD: Spec(b" ", [b"k1", b"k10", b"k100k1"], [b"1k1", b"0k10", b"kkk100"], [b"k", b"k0", b"100", b"kk"], None),
    LONG: Spec(b" ", [b"bd", b"bacd", b"bacacd"], [b"abd", b"cabacd", b"dbcd"], [b"bac", b"acd", b"bab"], None),
    EMAIL: Spec(b" ", [b"a@b", b"x.y@z.w"], [b"@a@b", b".@@q@r1"], [b"a@", b"@b", b"ab.c"], None),
    GLOBAL_FORM: Spec(b" ", [_H, b"bb" + _H], [b"x" + _H, b"bx" + _H], [b"abababx", b"b" * 14 + b"x"],
                      [b"xbab" + _H, b"x" + _H, b"xa" + _H, b"xab" + _H]),
    BOUNDED: Spec(b" ", [b"b", b"ca", b"aaab"], [b"ab", b"aab", b"acab"], [b"a", b"aaa", b"c", b"cc"], None),
}
EMPTY_ACCEPTING = ("a*", "x?y?z?")

Case = namedtuple("Case", "data lines first_want all_want starts placed")     # the first four: what a runner needs


def cell(b):
    return ("c", bytes(b))


def gap(n, sep=b" "):
    return ("s", sep * n)


def raw(b):
    """Inert bytes: no match contains them (a separator, NUL, a byte >= 0x80)."""
    return ("s", bytes(b))


def known(b, matches):
    """A part whose matches are known by construction, relative to its first byte."""
    return ("k", bytes(b), tuple(matches))


def line_bytes(parts):
    return b"".join(p[1] for p in parts)


class Cells:
    """The oracle's brute force per cell: all matches, relative to the cell.  One instance per pattern, answers kept."""
    _of = {}

    @classmethod
    def of(cls, pattern):
        if pattern not in cls._of:
            cls._of[pattern] = cls(pattern)
        return cls._of[pattern]

    def __init__(self, pattern):
        self.pattern, self.oracle, self.memo, self.needles = pattern, OracleRegex(pattern), {}, set()

    def learn(self, cells):
        new = sorted({c for c in cells if c not in self.memo})
        if not new:
            return
        assert all(0 < len(c) <= MAX_CELL and b"\n" not in c for c in new), "cells are short and hold no newline"
        cnt, st, en = self.oracle.search_all(b"\n".join(new) + b"\n")
        assert len(cnt) == len(new)
        k = 0
        for c, n in zip(new, cnt.tolist()):
            self.memo[c] = tuple((int(st[k + j]), int(en[k + j])) for j in range(n))
            k += n

    def matches(self, c):
        if c not in self.memo:
            self.learn([c])
        return self.memo[c]

    def confirm_needle(self, needle):
        """A needle is one match as a whole: accepted, and neither without its first byte nor without its last.  (The callers'
        needles hold their last byte once and their first byte once: no accepted substring ends earlier or starts later.)"""
        if needle not in self.needles:
            o = self.oracle
            assert o.accepts(needle.decode("latin-1")) and not o.accepts(needle[1:].decode("latin-1")) and not o.accepts(needle[:-1].decode("latin-1"))
            assert needle.count(needle[-1:]) == 1 and needle.count(needle[:1]) == 1
            self.needles.add(needle)


def check_parts(parts):
    """Two cells never touch: what lies between two matches of different cells is inert."""
    for a, b in zip(parts, parts[1:]):
        assert a[0] == "s" or b[0] == "s", "two cells without a separator between them"


def expectations(pattern, lines_parts):
    """-> (first_want, all_want): per line (start, end) of the first match or (-1, -1), and the list of all matches."""
    cells = Cells.of(pattern)
    cells.learn({p[1] for parts in lines_parts for p in parts if p[0] == "c"})
    memo, first_want, all_want = {}, [], []
    for parts in lines_parts:
        key = tuple(parts)
        if key not in memo:
            off, every = 0, []
            for p in parts:
                ms = cells.memo[p[1]] if p[0] == "c" else p[2] if p[0] == "k" else ()
                every += [(s + off, e + off) for s, e in ms]
                off += len(p[1])
            memo[key] = (every[0] if every else (-1, -1), every)
        first_want.append(memo[key][0])
        all_want.append(memo[key][1])
    return first_want, all_want


def empty_expectations(lines):
    """A pattern that accepts the empty string: [0, 0) first, [p, p) for p = 0 .. len."""
    return [(0, 0)] * len(lines), [[(p, p) for p in range(len(ln) + 1)] for ln in lines]


def assemble(pattern, lines_parts, final_newline, placed=()):
    """The corpus of these lines ('\\n' between them, one behind the last if final_newline) with its expectation."""
    lines = [line_bytes(p) for p in lines_parts]
    assert lines and (final_newline or lines[-1]), "a corpus without a final newline ends in a line that is not empty"
    for parts in lines_parts:
        check_parts(parts)
    data = np.frombuffer(b"\n".join(lines) + (b"\n" if final_newline else b""), dtype=np.uint8).copy()
    starts = np.concatenate([[0], np.cumsum([len(ln) + 1 for ln in lines])[:-1]]).astype(np.int64)
    first_want, all_want = expectations(pattern, lines_parts)
    case = Case(data, lines, first_want, all_want, starts, list(placed))
    verify_placements(case)
    return case


def verify_placements(case):
    """Every placement is where it was asked for, read off the finished corpus and its expectation."""
    data, starts = case.data, case.starts
    for p in case.placed:
        at, i, name = p["at"], p["line"], p["name"]
        assert at % p["modulus"] == p["residue"], p
        rel = at - int(starts[i])
        if name == "line_start":
            assert rel == 0 and (at == 0 or data[at - 1] == 10), p
        elif name == "newline":
            assert data[at] == 10 and rel == len(case.lines[i]), p
        elif name == "match_end":
            assert rel + 1 in {e for _, e in case.all_want[i]}, p
        elif name == "match_start":
            assert rel in {s for s, _ in case.all_want[i]}, p
        elif name == "byte":
            assert data[at] == p["value"], p
        else:
            raise AssertionError(("unknown placement", p))
        if "behind_lane" in p:                           # the match ends so many bytes behind the last byte of the lane its line starts in
            assert at - (int(starts[i]) | (LANE - 1)) == p["behind_lane"], p
    return len(case.placed)


class CaseBuilder:
    def __init__(self, pattern, seed):
        self.pattern, self.spec, self.rng = pattern, SPECS[pattern], random.Random(seed)
        self.cells = Cells.of(pattern)
        self.size, self.lines, self.placed, self.requested = 0, [], [], 0

    def add(self, parts):
        self.lines.append(list(parts))
        self.size += sum(len(p[1]) for p in parts) + 1
        return len(self.lines) - 1

    def exact(self, n, kind=None):
        """A line of n bytes: a cell of a random kind (or of `kind`) and separators, or separators alone."""
        kind = kind or self.rng.choice(("lead", "inner", "miss", "miss", "none"))
        c = self.rng.choice(getattr(self.spec, kind)) if kind != "none" else b""
        if not c or len(c) > n:
            return [gap(n, self.spec.sep)] if n else []
        front = self.rng.randint(0, n - len(c)) if kind != "lead" else 0
        return [p for p in (gap(front, self.spec.sep), cell(c), gap(n - len(c) - front, self.spec.sep)) if p[1]]

    def skip_to(self, start):
        """Short lines until the next line starts at the absolute offset `start`."""
        assert start >= self.size
        while start - self.size > 96:
            self.add(self.exact(self.rng.randint(0, 60)))
        if start > self.size:
            self.add(self.exact(start - self.size - 1))
        assert self.size == start

    def place(self, name, parts, feature, residue, modulus, **more):
        """The line `parts`, started where its byte `feature` (len: its '\\n') lies at `residue` mod `modulus`."""
        self.requested += 1
        start = self.size + (residue - self.size - feature) % modulus
        self.skip_to(start)
        i = self.add(parts)
        self.placed.append(dict(name=name, at=start + feature, line=i, residue=residue, modulus=modulus, **more))
        return i

    def match_of(self, c, k=0):
        return self.cells.matches(c)[k]

    def finish(self, final_newline=True):
        assert len(self.placed) == self.requested, "a requested placement was not produced"
        self.add(self.exact(17, "miss"))
        return assemble(self.pattern, self.lines, final_newline, self.placed)


# ---------------------------------------------------------------------------------------------------------------- a. residues
FOLLOW_DISTANCES = (1, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1)
FOLLOW_HITS = (4, 5, 9)                                  # kFollowHits = 4: as many, one more, many more


def residue_case(pattern, step=1, seed=11, final_newline=True):
    """One target per line (see the module text); step > 1 takes every step-th lane offset plus the edges of the lane and of its
    event words."""
    b = CaseBuilder(pattern, seed)
    sp, sep = b.spec, b.spec.sep
    lead, inner, miss = sp.lead[0], sp.inner[0], sp.miss[0]
    offs = sorted(set(range(0, LANE, step)) | {0, 1, 2, 3, 15, 16, 17, 127, 128, 129, 239, 240, 241, 253, 254, 255})
    last_lane = CHUNK - LANE
    starts = [[cell(lead), gap(2, sep)], [gap(1, sep), cell(inner)], [cell(miss), gap(1, sep), cell(miss)], []]
    # a line start at every offset of a lane; in lane 0 and in lane 63 of a chunk
    for k, r in enumerate(offs):
        b.place("line_start", starts[k % 4], 0, r, LANE)
    for k, r in enumerate((0, 1, 255, 256, last_lane, last_lane + 1, last_lane + 255)):
        b.place("line_start", starts[k % 3], 0, r, CHUNK)
    # a '\n' as a lane's and as a chunk's last byte, the line behind it with a match (it starts at the next lane's first byte)
    for modulus in (LANE, CHUNK):
        for k, parts in enumerate(([gap(3, sep), cell(inner)], [cell(miss)], [])):
            b.place("newline", parts, len(line_bytes(parts)), modulus - 1, modulus)
            b.add([cell(lead)] if k % 2 else [gap(1, sep), cell(inner), gap(1, sep), cell(lead)])
    # a match end at every byte of a lane: all sixteen of an event word, the first and the last word of the lane among them
    for k, r in enumerate(offs):
        parts = [gap(1 + r % 3, sep), cell(inner)] if k % 2 else [cell(lead), gap(1, sep), cell(miss)]
        front = len(parts[0][1]) if k % 2 else 0
        b.place("match_end", parts, front + b.match_of(inner if k % 2 else lead)[1] - 1, r, LANE)
    # match start x match end mod 4 (the walk's first word and its bound)
    combos = set()
    for s4 in range(WALK):
        for c in sp.sized:
            s, e = b.match_of(c)
            b.place("match_start", [gap(2, sep), cell(c), gap(1, sep), cell(c)], 2 + s, 64 + s4, LANE)
            combos.add((s4, (64 + s4 + e - s - 1) % WALK))
    assert len(combos) == 16, "every pair of residues mod 4 of a match's first and last byte"
    # a walk back over a lane boundary and over a chunk boundary, in a line that began before it
    longest = max(sp.sized, key=lambda c: b.match_of(c)[1] - b.match_of(c)[0])
    s, e = b.match_of(longest)
    for modulus in (LANE, CHUNK):
        for k in range(min(4, e - s - 1)):
            b.place("match_end", [gap(40, sep), cell(longest), gap(1, sep), cell(miss)], 40 + e - 1, k, modulus, crosses=modulus)
    # a match end D bytes behind the last byte of the lane its line starts in: the follow loop inside the chunk (owner in lane 0), into the
    # next chunk and over two chunks (owner in lane 63)
    h = len(inner) + 2
    ie = b.match_of(inner)[1]
    for owner in (LANE - h, CHUNK - h):
        for d in FOLLOW_DISTANCES:
            front = h + d - len(inner) + (len(inner) - ie)       # the match's last byte at line offset h - 1 + d
            parts = [gap(front, sep), cell(inner), gap(2, sep), cell(lead)]
            b.place("match_end", parts, h - 1 + d, (owner + h - 1 + d) % CHUNK, CHUNK, behind_lane=d)
    # more hits than the counting pass remembers in the followed stretch of an open last line
    for n in FOLLOW_HITS:
        parts = [gap(2, sep)] + [cell(inner), gap(1, sep)] * n
        assert 2 + b.match_of(inner)[1] > 6
        b.place("line_start", parts, 0, LANE - 6, LANE, follow_hits=n)
    return b.finish(final_newline)


def bounded_walk_case(seed=67):
    """BOUNDED, all matches: "ca" + k times 'a' + "b" is "ca", then a match that ends at the 'b' and may not start inside "ca" although
    "aaab" from the 'a' of "ca" is accepted when k is a multiple of 3.  The walk back takes four bytes per turn with a bound per byte:
    every k up to 16 with the match end at every residue mod 4 puts the bound at each of the four bytes of a turn (k = 3, 15: the
    accepted start one byte below the bound is the turn's fourth byte)."""
    b = CaseBuilder(BOUNDED, seed)
    sep = b.spec.sep
    for k in range(17):
        c = b"ca" + b"a" * k + b"b"
        for r in range(WALK):
            end = b.match_of(c, -1)[1]
            b.place("match_end", [gap(3, sep), cell(c), gap(1, sep), cell(c)], 3 + end - 1, 32 + r, LANE, tail_as=k)
    case = b.finish()
    assert any(len(w) == 4 and w[1][0] > w[0][1] for w in case.all_want) and any(len(w) == 4 and w[1][0] == w[0][1] for w in case.all_want)
    return case


# ------------------------------------------------------------------------------------------------------------- b. end of data
END_LENGTHS = (tuple(range(1, 41)), tuple(range(250, 261)), tuple(range(16380, 16401)), tuple(range(CHUNK + 250, CHUNK + 263)))
END_VARIANTS = ("as_cut", "final_newline", "match_at_end", "open_unmatched")


def end_of_data_base(pattern, seed=23):
    b = CaseBuilder(pattern, seed)
    while b.size < CHUNK + LANE + 64:
        b.add(b.exact(b.rng.choice((0, 1, 2, 3, 5, 8, 13, 21, 34, 55))))
    return b.lines


def cut_lines(lines_parts, n):
    """The first n bytes of the corpus (every line with its '\\n') -> (lines, whether the n-th byte is a '\\n' or n is 0)."""
    out, left = [], n
    for parts in lines_parts:
        if left == 0:
            return out, True
        cur = []
        for p in parts:
            assert p[0] != "k"
            take = p[1][:left]
            if take:
                cur.append((p[0], take))
            left -= len(take)
            if len(take) < len(p[1]):
                break
        out.append(cur)
        if left == 0:
            return out, False                            # the data ends inside this line or right in front of its '\n'
        left -= 1
    assert left == 0, "the base corpus is too short"
    return out, True


def end_of_data_case(pattern, base, n, variant):
    """n bytes of `base` (a slice: no byte moves), or None where n bytes cannot hold the variant."""
    sp = SPECS[pattern]
    if variant == "as_cut":
        lines, nl = cut_lines(base, n)
        if nl:                                           # ends in '\n': the line in front of it may be empty
            return assemble(pattern, lines, True)
        return assemble(pattern, lines, False)
    if variant == "final_newline":
        lines, nl = cut_lines(base, n - 1)
        return assemble(pattern, lines + [[]] if nl else lines, True)
    tail = [cell(sp.lead[0])] if variant == "match_at_end" else None
    if tail is None:
        k = min(n, 1 + n % 7)
        m = sp.miss[0]
        tail = [gap(k, sp.sep)] if k < len(m) + 1 else [gap(k - len(m), sp.sep), cell(m)]
    elif n % 2 and n > len(sp.inner[0]) + 2:
        tail = [gap(1, sp.sep), cell(sp.inner[0])]
    k = len(line_bytes(tail))
    if n < k:
        return None
    if n == k:
        return assemble(pattern, [tail], False)
    lines, nl = cut_lines(base, n - k - 1)
    case = assemble(pattern, (lines + [[]] if nl else lines) + [tail], False)
    if variant == "match_at_end":
        assert case.all_want[-1] and case.all_want[-1][-1][1] == len(case.lines[-1])
    else:
        assert not case.all_want[-1] and case.lines[-1]
    return case


# --------------------------------------------------------------------------------------------------------- c. staging length
STAGE_MULTIPLES = tuple(range(128, 2048 + 1, 64))
STAGE_PIECES = (STAGE_MULTIPLES[:11], STAGE_MULTIPLES[11:18], STAGE_MULTIPLES[18:25], STAGE_MULTIPLES[25:])


def staging_case(pattern, multiples=STAGE_MULTIPLES, pad=None):
    """Consecutive chunks own m - 1, m, m + 1, m + 2 lines for every m of `multiples`: short lines, every third with a match, the chunk's
    last line open, with a cell across the chunk boundary (every other one a match).  pad "plain": one newline-free line of whole chunks
    behind, until the corpus has fewer than 100 lines per chunk; pad "multi": chunks of 2-byte lines until it has more than 1650."""
    sp, sep = SPECS[pattern], SPECS[pattern].sep
    hits = (sp.lead[0], sp.inner[0])
    over = (sp.inner[0], sp.miss[-1])
    lines, owned, size, spill, t = [], [], 0, 0, 0
    for m in multiples:
        for n in (m - 1, m, m + 1, m + 2):
            assert size % CHUNK == spill
            last = [gap(2, sep), cell(over[len(owned) % 2]), gap(1, sep)]
            budget = CHUNK - spill - 3                   # the n - 1 whole lines with their '\n'; the last line has 3 bytes here
            kinds = [hits[(j // 3) % 2] if j % 3 == 0 else b"" for j in range(n - 1)]
            slack = budget - sum(max(len(c), 1) + 1 for c in kinds)
            assert slack >= 0, (pattern, n, "the lines do not fit the chunk")
            q, r = divmod(slack, n - 1)
            for j, c in enumerate(kinds):
                extra = q + (1 if j < r else 0)
                if c:
                    lines.append([cell(c), gap(extra, sep)] if extra else [cell(c)])
                else:
                    lines.append([gap(1 + extra, sep)] if (j + t) % 2 or 1 + extra < len(sp.miss[0]) else [cell(sp.miss[0]), gap(1 + extra - len(sp.miss[0]), sep)])
            lines.append(last)
            size += budget + len(line_bytes(last)) + 1
            spill = size % CHUNK
            assert spill == len(line_bytes(last)) + 1 - 3
            owned.append(n)
            t += 1
    lines.append([gap(5, sep), cell(hits[0])])
    size += 5 + len(hits[0]) + 1
    nchunks = len(owned) + 1
    if pad == "plain":
        target = len(lines) // 100 + 2                   # chunks the corpus must have
        n = (target - nchunks) * CHUNK + (CHUNK - size % CHUNK)
        lines.append([gap(n, sep)])
        size += n + 1
    elif pad == "multi":
        extra = 1
        while (len(lines) + extra * (CHUNK // 2)) / (nchunks + extra) <= 1650:
            extra += 1
        lines += [[gap(1, sep)] if j % 5 else [cell(sp.miss[0][:1])] for j in range(extra * (CHUNK // 2) + 7)]
    case = assemble(pattern, lines, True)
    per_chunk = np.bincount(case.starts // CHUNK, minlength=len(owned))
    assert per_chunk[:len(owned)].tolist() == owned, "every chunk owns the requested number of lines"
    mean = len(case.lines) / ((len(case.data) + CHUNK - 1) // CHUNK)
    assert pad != "plain" or mean < 100
    assert pad != "multi" or mean > 1650
    return case, owned


# ----------------------------------------------------------------------------------------------------------- d. packing limits
PACK_OFFSETS = (0x7ffe, 0x7fff, 0x8000, 0x8001, 0xfffe, 0xffff, 0x10000, 0x1ffef, 0x1fff0, 0x1fff1)


def needle(pattern, n):
    """One match of n bytes."""
    assert n >= 3
    return {LONG: b"b" + (b"ac" * n)[:n - 2] + b"d", "ab+c": b"a" + b"b" * (n - 2) + b"c"}[pattern]


def packing_case(pattern, long_walk, offsets=PACK_OFFSETS, seed=31):
    """Lines whose first match ends `offset` bytes behind the line start: a needle that starts at the line's second byte (a walk of the
    whole length) and, for some, at its first (no walk), or a short cell behind separators; further matches follow it."""
    b = CaseBuilder(pattern, seed)
    sp, sep = b.spec, b.spec.sep
    inner, lead = sp.inner[0], sp.lead[0]
    tail = [gap(1, sep), cell(lead), gap(2, sep), cell(inner), gap(1, sep)]
    for k, end in enumerate(offsets):
        heads = []
        if long_walk:
            heads.append([gap(1, sep), known(needle(pattern, end - 1), [(0, end - 1)])])
            if k % 3 == 2:
                heads.append([known(needle(pattern, end), [(0, end)])])
        else:
            heads.append([gap(end - b.match_of(inner)[1], sep), cell(inner)])
        for head in heads:
            for p in head:
                if p[0] == "k":
                    b.cells.confirm_needle(p[1])
            b.requested += 1
            i = b.add(head + tail)
            at = b.size - len(line_bytes(head + tail)) - 1 + end - 1
            b.placed.append(dict(name="match_end", at=at, line=i, residue=0, modulus=1, from_line_start=end))
            b.add(b.exact(b.rng.randint(0, 40)))
    case = b.finish()
    for p in case.placed:
        assert case.first_want[p["line"]][1] == p["from_line_start"], "the first match ends where the case says"
    return case


def dense_line_case(n=20480):
    """KEYWORD on a line of n times "k1": every second byte ends a match, more than any staging array holds."""
    text = b"k1" * n
    cells = Cells.of(KEYWORD)
    assert cells.matches(b"k1k1k1") == ((0, 2), (2, 4), (4, 6))
    ends = np.arange(2, 2 * n + 1, 2)
    sp = SPECS[KEYWORD]
    lines = [[cell(sp.lead[1])], [gap(3), known(text, zip((ends - 2).tolist(), ends.tolist())), gap(2), cell(sp.inner[0])], [cell(sp.miss[1])],
             [cell(sp.inner[1]), gap(1), cell(sp.lead[0])]]
    return assemble(KEYWORD, lines, True)


# -------------------------------------------------------------------------------------------------------------- e. dense walks
def dense_walks_case(pattern, seed=41):
    """Matches that need a walk back, packed: (1) a chunk of short lines, one per line - more lines than any staging array holds, so the
    hits go through the wave's pool one by one; (2) lines of a dozen bytes - parked, then pooled 64 at a time; (3) long lines of cells a
    separator apart - hundreds of hits in flight; (4) 64 lines of 255 bytes that start six bytes before a lane's end, so every lane of a
    wave follows its open line at once, a hit every few bytes."""
    b = CaseBuilder(pattern, seed)
    sp, sep = b.spec, b.spec.sep
    walks = sp.inner
    shortest = min(walks, key=len)
    for j in range(6000):
        b.add([cell(shortest)] if j % 7 else [cell(sp.miss[0])])
    for j in range(1500):
        b.add([gap(1 + j % 5, sep), cell(walks[j % len(walks)]), gap(j % 3, sep)] if j % 5 else [gap(2, sep), cell(sp.miss[1])])
    for j in range(40):
        b.add([p for k in range(120) for p in (cell(walks[(j + k) % len(walks)]), gap(1, sep))])
    unit = [cell(walks[0]), gap(1, sep)]
    n = (LANE - 1 - 2) // len(line_bytes(unit))
    body = [gap(2, sep)] + unit * n
    body.append(gap(LANE - 1 - len(line_bytes(body)), sep))
    b.place("line_start", body, 0, LANE - 6, CHUNK)
    for _ in range(2 * 64):
        b.add(body)
    return b.finish()


# ------------------------------------------------------------------------------------------------------ f. high bytes and NUL
ODD_BYTES = (0x80, 0xff, 0x00, 0xc3)


def odd_bytes_case(pattern, seed=53):
    """A byte >= 0x80 or a NUL at every offset of an event word (so: as either byte of a pair, in each of the four text words) directly in
    front of a match (the walk back steps on it) and directly behind one, as a lane's last byte, and in the stretch a lane follows."""
    b = CaseBuilder(pattern, seed)
    sp, sep = b.spec, b.spec.sep
    inner, lead = sp.inner[0], sp.lead[0]
    for r in range(WORD):
        for v in ODD_BYTES:
            x = raw(bytes([v]))
            b.place("byte", [gap(3, sep), x, cell(inner), gap(1, sep), cell(lead)], 3, r, WORD, value=v)
            b.place("byte", [gap(2, sep), cell(inner), x, cell(lead), x], 2 + len(inner), r, WORD, value=v)
            b.place("byte", [x, cell(lead), x, x, cell(inner)], 0, r, WORD, value=v)
    for v in ODD_BYTES:
        x = raw(bytes([v]))
        b.place("byte", [gap(4, sep), x, cell(inner), gap(1, sep)], 4, LANE - 1, LANE, value=v)
        b.place("byte", [gap(4, sep), cell(inner), x], 4 + len(inner), LANE - 1, LANE, value=v)
        for r in range(WORD):                            # the line starts six bytes before the lane's end; the byte lies 8 + r behind its start
            parts = [gap(8 + r, sep), x, cell(inner), x, gap(1, sep), cell(lead)]
            start = b.size + (LANE - 6 - b.size) % LANE
            b.place("byte", parts, 8 + r, (start + 8 + r) % LANE, LANE, value=v)
    case = b.finish()
    assert int((case.data >= 0x80).sum()) > 100 and int((case.data == 0).sum()) > 50
    return case


def single_high_byte_case(pattern, seed=59):
    """Ordinary short lines and exactly one byte >= 0x80, in a line without a match, a lane away from every match."""
    b = CaseBuilder(pattern, seed)
    while b.size < 3 * CHUNK // 2:
        b.add(b.exact(b.rng.randint(0, 70)))
    b.place("byte", [gap(300, b.spec.sep), raw(b"\x80"), gap(300, b.spec.sep)], 300, 7, WORD, value=0x80)
    while b.size < 3 * CHUNK:
        b.add(b.exact(b.rng.randint(0, 70)))
    case = b.finish()
    assert int((case.data >= 0x80).sum()) == 1
    return case


# ---------------------------------------------------------------------------------------------- h. patterns that accept ""
def empty_case(stripe, final_newline, seed=61):
    rng = random.Random(seed + stripe)
    lengths = [0, 1, stripe - 1, stripe, stripe + 1, 3 * stripe + 7]
    order = lengths + [lengths[k] for k in (5, 0, 3, 0, 1, 2, 4)] + [9]
    lines = [bytes(rng.choice(b"axyz q") for _ in range(n)) for n in order]
    data = np.frombuffer(b"\n".join(lines) + (b"\n" if final_newline else b""), dtype=np.uint8).copy()
    starts = np.concatenate([[0], np.cumsum([len(ln) + 1 for ln in lines])[:-1]]).astype(np.int64)
    first_want, all_want = empty_expectations(lines)
    return Case(data, lines, first_want, all_want, starts, [])


# ------------------------------------------------------------------------- the route for patterns without a separator
def _oracle_confirms_search(pattern, lines, first=None, every=None, seed=1, starts_per_match=10):
    """Search results against the ORACLE's own compile of the pattern, not against a replay of the device's tables.  With
    `contains` = the oracle's automaton of `.*(p).*` (`.` covers all 128 codes, Parser.cpp:106-109) and `o` that of p:
      * a line reported without a match: `contains` rejects the whole line (no substring is accepted);
      * a match [s, e) searched from position b: o accepts line[s:e]; `contains` rejects line[b:e-1] (no match ends earlier - a
        complete check, one oracle run); no s' in a sample of [b, s) (always b, s-1, s-2) has line[s':e] accepted.
    `first`: one (s, e) per line; `every`: the list of all matches per line, each searched from the end of the one before."""
    rng = random.Random(seed)
    o, contains = OracleRegex(pattern), OracleRegex(".*(" + pattern + ").*")

    def confirm(ln, b, s, e):
        assert b <= s <= e <= len(ln), (pattern[:30], b, s, e)
        assert o.accepts(ln[s:e].decode("latin-1")), (pattern[:30], "not a match", s, e)
        if e - 1 >= b:
            assert not contains.accepts(ln[b:e - 1].decode("latin-1")), (pattern[:30], "a match ends before", e)
        for s2 in {b, s - 1, s - 2} | {rng.randrange(b, s) for _ in range(starts_per_match) if s > b}:
            if b <= s2 < s:
                assert not o.accepts(ln[s2:e].decode("latin-1")), (pattern[:30], "an earlier start", s2, "for", (s, e))

    for i, ln in enumerate(lines):
        if first is not None:
            s, e = first[i]
            if e < 0:
                assert not contains.accepts(ln.decode("latin-1")), (pattern[:30], "line", i, "has a match")
            else:
                confirm(ln, 0, s, e)
        if every is not None:
            b = 0
            for s, e in every[i]:
                confirm(ln, b, s, e)
                b = e if e > s else e + 1                       # (an empty match: the search moves on by one byte)
            if b <= len(ln):
                assert not contains.accepts(ln[b:].decode("latin-1")), (pattern[:30], "line", i, "has a further match after", b)
