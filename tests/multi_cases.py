"""Pattern sets, items and oracles shared by the tests of rrx_multi (tests/test_multi_contains_lowering.py on the CPU,
tests/test_multi_contains_gpu.py on the device): bit k of an item's mask = the item contains a match of member k.

The sets are drawn from contains_cases.FIXED - every one of those patterns has a contains table, so no member is ever refused -
plus one set with '\\n' inside its patterns.  The items are those of test_contains_items_lowering.short_items, drawn once per
member and laid end to end: every member of a set sees the items planted for every other member too.  The brute force runs once
per (pattern, item list) and is shared by every set that holds the pattern."""
import random

import numpy as np

from contains_cases import FIXED
from patterns import EMAIL, U2
from test_contains_items_lowering import NEWLINE_PATTERNS, as_oracle_sees, contains_brute_force, oracle_for, short_items

# name -> members.  Sizes 1, 2, 5, 12 and 32; a nullable member ("a*", "x?y?z?"), a duplicate, '\n' in a pattern.  In every set of
# two members or more some neighbours cannot share a table of 16 rows: max_rows of 8 and of 16 must cut it into two groups at least.
SETS = {
    "one": [FIXED[0]],
    "two": ["(a|b)*abb", U2],
    "five": ["ab+c", "(a|b)*abb", "[0-9]+\\.[0-9]+", "k(1|10|100)", EMAIL],
    "twelve": list(FIXED),
    "thirtytwo": (FIXED * 3)[:32],
    "nullable": ["a*", "ab+c", "(a|b)*abb", "[0-9]+\\.[0-9]+", EMAIL],
    "duplicate": ["ab+c", "k(1|10|100)", "ab+c", "a{2,4}b", "[^a]b", EMAIL],
    "newline": ["ab+c", "a\nb", "k\n+1", "(a|b|\n)*ab(a|\n)*", "k(1|10|100)", "a{2,4}b"],
}
assert sorted(len(v) for v in SETS.values()) == [1, 2, 5, 5, 6, 6, 12, 32]
assert all(p in FIXED or p in NEWLINE_PATTERNS for v in SETS.values() for p in v)

_cache = {}


def fixed_items():
    """36 short items per pattern of FIXED, in FIXED's order (432 items of at most 22 bytes)."""
    if "fixed" not in _cache:
        rng = random.Random(3301)
        _cache["fixed"] = [it for p in FIXED for it in short_items(rng, p, 36)]
    return _cache["fixed"]


def newline_items():
    """Items for the set with '\\n' in its patterns: the oracle's dialect cannot spell the byte and reads 'x' in its place, so these
    items are drawn over the alphabet without 'x' (test_contains_items_lowering.NEWLINE_ALPHABET), for the three '\\n' patterns, plus
    a few written by hand for the members that have no '\\n'."""
    if "newline" not in _cache:
        rng = random.Random(3302)
        items = [it for p in NEWLINE_PATTERNS for it in short_items(rng, p, 60)]
        items += [b"abbc", b"a\nbk100", b"k\n\n1aab", b"zk10\naaab", b"ab\nab\nc", b"", b"\n", b"aab\xffa\nb\x00k1"]
        assert not any(b"x" in it for it in items)
        _cache["newline"] = items
    return _cache["newline"]


def items_of(name):
    return newline_items() if name == "newline" else fixed_items()


def want_column(p, which):
    """uint8 per item of the list `which` ("fixed" / "newline"): the brute force over the item's substrings for pattern p."""
    key = (p, which)
    if key not in _cache:
        o = oracle_for(p)
        items = newline_items() if which == "newline" else fixed_items()
        _cache[key] = np.array([contains_brute_force(o, as_oracle_sees(p, it)) for it in items], dtype=np.uint8)
    return _cache[key]


def want_masks(name):
    """uint32 per item: bit k = want_column of member k.  (A fresh array per call: callers may not change what the cache holds.)"""
    which = "newline" if name == "newline" else "fixed"
    m = np.zeros(len(items_of(name)), dtype=np.uint32)
    for k, p in enumerate(SETS[name]):
        m |= want_column(p, which).astype(np.uint32) << np.uint32(k)
    return m


class MultiReplay:
    """One group's table from rrx_multi_program_words: [nstates, ncls, start, first_hit, full], cls[256], next[nstates][ncls],
    mask[nstates]."""

    def __init__(self, words):
        w = np.asarray(words, dtype=np.uint32)
        self.nstates, self.ncls, self.start, self.first_hit, self.full = (int(x) for x in w[:5])
        self.cls = w[5:261].astype(np.int64)
        n = self.nstates * self.ncls
        self.next = w[261:261 + n].astype(np.int64).reshape(self.nstates, self.ncls)
        self.mask = w[261 + n:261 + n + self.nstates]
        assert w.size == 261 + n + self.nstates

    def item_mask(self, item):
        """As the kernel steps it: the start row's mask, then every byte; the mask is read on rows from first_hit on only, and the
        walk stops once nothing more can be found."""
        s = self.start
        m = int(self.mask[s])
        for c in item:
            if m == self.full:
                break
            s = int(self.next[s, self.cls[c]])
            if s >= self.first_hit:
                m |= int(self.mask[s])
        return m


def replay(multi, items):
    """uint32 per item: the OR of the groups' masks."""
    groups = [MultiReplay(multi.program(g)) for g in range(multi.groups)]
    return np.array([sum_or(g.item_mask(it) for g in groups) for it in items], dtype=np.uint32)


def sum_or(values):
    m = 0
    for v in values:
        m |= v
    return m


def pack_items(items, trim=0, lead=0, sep=b"\n"):
    """(bytes uint8, offsets int64) of a batch: `lead` bytes of filler first, every item followed by `trim` separator bytes."""
    buf = bytearray(b"#" * lead)
    off = [lead]
    for it in items:
        buf += it + sep * trim
        off.append(len(buf))
    return np.frombuffer(bytes(buf), dtype=np.uint8).copy(), np.array(off, dtype=np.int64)
