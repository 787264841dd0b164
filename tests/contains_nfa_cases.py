"""The case table of contains on the NFA lane engine (RRX_OPT_CONTAINS_NFA; kernels_nfa.inc: ContainsLineNfaEngine,
contains_extents_nfa_kernel), shared by test_contains_nfa_lowering.py (no GPU: the dumps, the replay) and test_contains_nfa_gpu.py
(the kernels against the same vectors).  Needs neither a GPU nor torch.

Built on nfa_width_cases.CASES: for each of them the pattern is x(p)y, and a line is one to three SEGMENTS x + t + y, t drawn from
nfa_width_cases.lines(case) - members and near misses around every accept edge and word boundary -, with junk in front, between and
behind: letters of the case's alphabet and, sometimes, a two-byte UTF-8 character, a NUL, a stray x or a stray y (never an x and a
y in one piece of junk).  Neither x nor y is in any family's alphabet, so a match is exactly a segment whose t the pattern p
accepts as a whole string: the expected bit of a line is the OR over its segments of the RECORDED oracle verdict
nfa_width_cases.expected(case) of t (0 for a t that holds a NUL or a high byte: the oracle rejects it).  The verdict depends on
the program's deepest positions, and it needs neither a golden file of its own nor the slow oracle.

x(p)y has two positions more than p, and the lane engine holds 512: the four cases of 512 positions (TOO_LARGE) have no lane program
as x(p)y.  They are not run; test_contains_nfa_lowering.py holds them to RRX_ERR_UNSUPPORTED instead.

Beside them the patterns WITHOUT a contains table (TABLELESS): their lines are runs of a/b cut by '-', their expectation the oracle's
own automaton of .*(p).* on those ASCII lines (contains_cases.dot_star)."""
import random
from collections import namedtuple

import numpy as np

import nfa_width_cases as W

Case = namedtuple("Case", "id base pattern")

MAX_LANE_POSITIONS = 512
CASES = [Case("contains-" + c.id, c, "x(" + c.pattern + ")y") for c in W.CASES if c.nbits + 2 <= MAX_LANE_POSITIONS]
TOO_LARGE = [Case("contains-" + c.id, c, "x(" + c.pattern + ")y") for c in W.CASES if c.nbits + 2 > MAX_LANE_POSITIONS]
SOURCE_LINES = 240                                         # segments per case
MAX_CORPUS_BYTES = 300 << 10

_built = {}


def _junk(rng, alphabet, stray_ok=True):
    out = bytearray("".join(rng.choice(alphabet) for _ in range(rng.choice((0, 0, 1, 3, 9)))).encode())
    k = rng.random()
    special = b"\xc3\xa9" if k < 0.12 else b"\x00" if k < 0.24 else b"x" if k < 0.36 and stray_ok else b"y" if k < 0.48 and stray_ok else b""
    at = rng.randint(0, len(out))
    return bytes(out[:at] + special + out[at:])


def _sources(case):
    """indices into nfa_width_cases.lines(base): the longest accepted lines (they end in the top word), the lines of the edge lengths,
    the two lines with a NUL / a high byte, and a random rest"""
    base = case.base
    ls, exp = W.lines(base), W.expected(base)
    rng = random.Random(case.id)
    accepted = sorted((i for i in range(len(ls)) if exp[i]), key=lambda i: -len(ls[i]))
    bad = [i for i, t in enumerate(ls) if any(c == 0 or c >= 0x80 for c in t)]
    picked = list(dict.fromkeys(accepted[:50] + W.edge_lines(base) + bad))
    rest = [i for i in range(len(ls)) if i not in set(picked)]
    rng.shuffle(rest)
    return (picked + rest)[:SOURCE_LINES], rng


def build(case):
    """-> (lines: list of bytes without '\\n', expected: numpy uint8 per line, read-only); the same on every call"""
    if case.id in _built:
        return _built[case.id]
    base = case.base
    ls, exp = W.lines(base), W.expected(base)
    src, rng = _sources(case)
    member = next(i for i in src if exp[i])                # the longest accepted line
    seg = lambda i: b"x" + ls[i] + b"y"
    # the fixed lines: a match behind a NUL, behind a high byte, behind junk, in front of junk, alone, and each again with a near miss
    lines = [b"\x00" + seg(member), b"\xc3\xa9" + seg(member), b"\x80" + seg(member), base.alphabet.encode() + seg(member), seg(member) + base.alphabet.encode(),
             seg(member), b"x" + seg(member), seg(member) + b"y", b"y" + seg(member) + b"x"]
    want = [1] * len(lines)
    lines += [b"", b"x", b"y", b"xy", b"x\x00y", b"x" + ls[member][:-1] + b"\x00" + ls[member][-1:] + b"y"]
    want += [0, 0, 0, 0, 0, 0]
    queue = list(src)
    k = 0
    while queue:
        n = 1 if k < 60 else rng.choice((1, 2, 2, 3))
        segs, queue = queue[:n], queue[n:]
        line = _junk(rng, base.alphabet)
        for j, i in enumerate(segs):
            line += seg(i) + _junk(rng, base.alphabet)
        lines.append(line)
        want.append(int(max(exp[i] for i in segs)))
        k += 1
    order = list(range(len(lines)))
    rng.shuffle(order)
    order.sort(key=lambda i: lines[i] == b"")              # (an empty line last but one: without a final '\n' an empty last line is no line)
    order.append(order.pop(0))
    lines = [lines[i] for i in order]
    want = np.array([want[i] for i in order], dtype=np.uint8)
    want.setflags(write=False)
    assert all(b"\n" not in t for t in lines) and lines[-1] != b""
    assert sum(len(t) + 1 for t in lines) <= MAX_CORPUS_BYTES
    _built[case.id] = (lines, want)
    return _built[case.id]


def corpus(case, final_newline=True):
    return b"\n".join(build(case)[0]) + (b"\n" if final_newline else b"")


def items(case, trim):
    """-> (data bytes, offsets numpy int64): the lines as items, each followed by `trim` separator bytes ('\\n' or ';')"""
    ls = build(case)[0]
    sep = b";" * trim
    off = np.zeros(len(ls) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(t) + trim for t in ls])
    return b"".join(t + sep for t in ls), off


# ---- the patterns without a contains table
TABLELESS = ["(a|b)*a(a|b){14}", "(a|b)*a(a|b){40}", "c(a|b)*a(a|b){128}d"]
_tableless = {}


def _run(rng, n, accept, lead):
    """an a/b run: `lead` random letters, the deciding letter, then n letters"""
    s = [rng.choice("ab") for _ in range(lead + 1 + n)]
    if accept:
        s[lead] = "a"
    else:                                                  # no 'a' with n letters or more behind it
        for i in range(0, len(s) - n):
            s[i] = "b"
    return "".join(s)


def tableless_lines(p):
    """ASCII lines for one of TABLELESS: runs of a/b (c + run + d for the third), members and near misses, cut by '-'"""
    if p in _tableless:
        return _tableless[p]
    n = int(p.rsplit("{", 1)[1].split("}")[0])
    framed = p.startswith("c")
    rng = random.Random(p)
    wrap = (lambda r: "c" + r + "d") if framed else (lambda r: r)
    out = ["", "-", "a", "b" * (n + 5), wrap("a" * (n + 1)), wrap("a" * n), wrap("a" + "b" * n), "c" + "a" * (n + 1), "a" * (n + 1) + "d",
           wrap("b" * 70 + "a" + "b" * n), wrap("a" + "b" * (n - 1)) + "-" + wrap("b" * n)]
    for k in range(150):
        runs = []
        for _ in range(rng.choice((1, 1, 2, 3))):
            r = _run(rng, n, rng.random() < 0.4, rng.choice((0, 1, 7, 33)))
            if rng.random() < 0.2:
                r = r[:rng.randint(0, len(r))]             # cut short: mostly a miss
            if framed and rng.random() < 0.15:
                r = r[:len(r) // 2] + rng.choice("cd") + r[len(r) // 2:]
            runs.append(wrap(r) if rng.random() < 0.85 else r)
        out.append(rng.choice(("", "-", "ab-")) + "-".join(runs) + rng.choice(("", "-", "-ba")))
    rng.shuffle(out)
    out.sort(key=lambda t: t == "")
    out.append(out.pop(0))
    _tableless[p] = [t.encode() for t in out]
    return _tableless[p]


_tableless_expected = {}


def tableless_expected(p):
    """uint8 per line of tableless_lines(p): the oracle's own automaton of .*(p).* accepts it"""
    if p not in _tableless_expected:
        from contains_cases import dot_star
        v = dot_star(p, tableless_lines(p))
        v.setflags(write=False)
        _tableless_expected[p] = v
    return _tableless_expected[p]


def unpack(bits, n):
    """int32 / uint32 bitmap words -> uint8 per line."""
    w = np.ascontiguousarray(bits).view(np.uint32)
    return ((w[np.arange(n) >> 5] >> (np.arange(n, dtype=np.uint32) & 31)) & 1).astype(np.uint8)
