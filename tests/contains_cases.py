"""Patterns, texts and oracles shared by the contains tests (tests/test_contains_lowering.py on the CPU, tests/test_contains_gpu.py
on the device): a line CONTAINS a match iff rrx_search_corpus would report one for it."""
import random

import numpy as np

from patterns import EMAIL, K1000_CONTAINS, U2, random_pattern
from pyoracle import OracleError, OracleRegex

FIXED = ["ab+c", "a*", "(a|b)*abb", "[0-9]+\\.[0-9]+", "x?y?z?", "k(1|10|100)", "a{2,4}b", ".*c", "c.*", "[^a]b", EMAIL, U2]
EXPLODING = "(a|b)*a(a|b){40}"                  # subset construction beyond the state budget: no contains table


def short_line_patterns():
    """The fixed list and the seed-77 random set of test_search_corpus_short_lines_against_the_oracle (random patterns with at
    most 120 reference states)."""
    rng = random.Random(77)
    pats = list(FIXED)
    while len(pats) < 40:
        p = random_pattern(rng)
        try:
            if OracleRegex(p).states_n <= 120:
                pats.append(p)
        except OracleError:
            pass
    return pats


def alphabet_for(p):
    return "ab1.@:/hftps" if p in (EMAIL, U2, K1000_CONTAINS) else "abcxk01.d@yz"


def short_lines(rng, p, n):
    """Lines of at most 22 bytes (the oracle's brute force is cubic), with NUL, 0x80, a two-byte UTF-8 character and empty lines."""
    a = alphabet_for(p)
    lines = ["".join(rng.choice(a) for _ in range(rng.choice([0, 0, 1, 2, 5, 9, 14, 20]))).encode() for _ in range(n)]
    lines[5] = (b"\x80ab" + lines[5])[:22]
    lines[9] = (lines[9][:10] + b"\xc3\xa9" + lines[10][:10])
    lines[12] = (lines[12][:8] + b"\x00" + lines[13][:8])
    lines[20] = b""
    for i in range(30, n, 17):                  # one line in 17 carries a high byte or a NUL somewhere
        ln = bytearray(lines[i][:20])
        ln.insert(rng.randint(0, len(ln)), rng.choice([0x00, 0x80, 0xff]))
        lines[i] = bytes(ln)
    return lines


def brute_force(p, data):
    """uint8 per line: the oracle's brute-force search finds a match."""
    return (OracleRegex(p).search_lines(data)[1] >= 0).astype(np.uint8)


def long_ascii_lines(rng, p, n, maxlen=3000):
    a = alphabet_for(p) + "   "
    return ["".join(rng.choice(a) for _ in range(rng.choice([30, 100, 700, maxlen]))).encode() for _ in range(n)]


def dot_star(p, lines):
    """uint8 per ASCII line: the oracle's own automaton of .*(p).* accepts it."""
    o = OracleRegex(".*(" + p + ").*")
    return np.array([o.accepts(ln.decode("latin-1")) for ln in lines], dtype=np.uint8)


def split_lines(data):
    data = bytes(data)
    lines = data.split(b"\n")
    return lines[:-1] if data.endswith(b"\n") or not data else lines


def unpack(bits, n):
    """int32 / uint32 bitmap words -> uint8 per line."""
    w = np.ascontiguousarray(bits).view(np.uint32)
    return ((w[np.arange(n) >> 5] >> (np.arange(n, dtype=np.uint32) & 31)) & 1).astype(np.uint8)
