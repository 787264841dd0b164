"""The case table of the NFA lane engine's width-by-build matrix (kernels_nfa.inc): every program width 1 ... 16 crossed with the
five program shapes the kernel builds are chosen from, with the lines each case is run on and the oracle's verdicts.  Shared by
test_nfa_widths_lowering.py (no GPU: the dumps are what this table says, the replay equals the oracle) and test_nfa_widths_gpu.py
(the kernels against the same vectors).  Needs neither a GPU nor torch.

    shape   family                          program (rrx_program_words)            batch build          one-pass build
    chain   a{1,n}                          self = 0, cgrp = 0, n_exc = 0          <W,0,0,0>            <W,0,0,0>
    self    a{n}b*, b+a{1,n}                self != 0, cgrp = 0, n_exc = 0         <W,1,0,0>            <W,1,0,1>
    carry   (a?){n}b, b*a{1,n},             cgrp != 0, n_exc = 0                   <W,1,0,1>            <W,1,0,1>
            (a|b)*a(a|b){n}
    exc     (ab|ba){1,k}                    n_exc > 0, cgrp = 0                    <W,1,1,0>, carry flag off
    mix     c*(ab|ba){1,k}(d|e)?f,          n_exc > 0, cgrp != 0                   <W,1,1,0>, carry flag on
            (ab|ba){1,k}c?d

Positions per family (checked by the lowering test): a{1,n}: n + 1; a{n}b*, b+a{1,n}, (a?){n}b, b*a{1,n}: n + 2; (a|b)*a(a|b){n}:
n + 3; (ab|ba){1,k}: 4k + 2; c*(ab|ba){1,k}(d|e)?f: 4k + 5; (ab|ba){1,k}c?d: 4k + 4.  Programs of 5, 7, 9-11 and 13-15 words run the
kernels built for 6, 8, 12 and 16 words on tables padded with zero words (pack.cpp: instantiated_width)."""
import hashlib
import json
import os
import random
from collections import namedtuple

Case = namedtuple("Case", "id shape family pattern alphabet W nbits n lengths")

KERNEL_WIDTHS = (1, 2, 3, 4, 6, 8, 12, 16)
BATCH_BUILDS = ("chain", "self", "carry", "exc")            # LineNfaEngine<W,0,0,0>, <W,1,0,0>, <W,1,0,1>, <W,1,1,0>
ONEPASS_BUILDS = ("chain", "selfcarry", "exc")              # LineNfaEngine<W,0,0,0>, <W,1,0,1>, <W,1,1,0>
# widths at which the chain a{1,n} is cut to nbits == 32 W (the top word's bit 31 in use, and final) and to nbits == 32 (W - 1) + 1
# (only bit 0 of the top word): the narrow kernels' ends, and a padded and an exact program in front of each wide kernel
EDGE_WIDTHS = (1, 2, 4, 5, 7, 8, 11, 12, 15, 16)


def kernel_width(W):
    """pack.cpp: instantiated_width"""
    return W if W <= 4 else 6 if W <= 6 else 8 if W <= 8 else 12 if W <= 12 else 16


def batch_build(n_exc, cgrp, self_):
    """match_stripes_nfa's choice (kernels_nfa.inc): any_exc ? exc : any_carry ? carry : any_self ? self : chain"""
    return "exc" if n_exc else "carry" if cgrp else "self" if self_ else "chain"


def onepass_build(n_exc, cgrp, self_):
    """match_onepass_nfa's choice: any_exc ? exc : (any_self || any_carry) ? self + carry : chain"""
    return "exc" if n_exc else "selfcarry" if (cgrp or self_) else "chain"


def _pairs(rng, j):
    return "".join(rng.choice(("ab", "ba")) for _ in range(j))


def _word_edges(limit):
    """lengths around every multiple of 32 up to `limit`"""
    return [L for k in range(1, limit // 32 + 2) for L in (32 * k - 2, 32 * k - 1, 32 * k, 32 * k + 1) if 0 <= L <= limit]


# ---- the families: pattern, positions, alphabet, lengths around the accept edges, members and near misses, a likely member of a length
def _chain_members(n, rng):
    out = ["a" * L for L in [0, 1, 2, n - 1, n, n + 1, n + 2] + _word_edges(n + 2)]
    return out + ["a" * (n - 1) + "b", "a" * max(n - 2, 0) + "ba", "b" + "a" * (n - 1)]


def _self_members(n, rng):
    return ["a" * n + "b" * j for j in (0, 1, 2, 40)] + ["a" * (n - 1), "a" * (n + 1), "a" * (n - 1) + "b", "a" * (n - 1) + "bb",
                                                       "a" * n + "ba", "a" * n + "bbba", "b" + "a" * n]


def _self2_members(n, rng):
    return ["b" * j + "a" * L for j in (1, 2, 35) for L in (0, 1, n - 1, n, n + 1)] + ["a" * n, "b" * 3 + "a" * (n - 1) + "b", "b" + "a" * n + "b"]


def _carry_members(n, rng):
    out = ["a" * L + "b" for L in [0, 1, n - 1, n, n + 1] + _word_edges(n)]
    return out + ["a" * n, "b", "bb", "a" * (n - 1) + "bb", "a" * n + "ba", "ab" + "a" * (n - 2) + "b"]


def _carry2_members(n, rng):
    out = ["b" * j + "a" * L for j in (0, 1, 40) for L in [0, 1, n - 1, n, n + 1]] + ["b" + "a" * L for L in _word_edges(n)]
    return out + ["b" * 2 + "a" * (n - 1) + "b", "a" * (n - 1) + "ba", "ab" + "a" * (n - 2)]


def _ab(rng, L):
    return "".join(rng.choice("ab") for _ in range(L))


def _carry3_members(n, rng):
    out = []
    for lead in (0, 1, 2, 50):
        for mark in "ab":                                   # the byte n + 1 from the end decides
            out += [_ab(rng, lead) + mark + _ab(rng, n), "b" * lead + mark + "b" * n, "a" * lead + mark + "a" * n]
    return out + ["a" * n, "a" * (n + 1), "b" * (n + 1), "a" + "b" * (n - 1), "ba" + "b" * (n - 1)]


def _exc_members(k, rng):
    out = []
    for j in [0, 1, 2, k - 1, k, k + 1]:
        out += [_pairs(rng, j), _pairs(rng, j), "ab" * j, "ba" * j]
    out += [_pairs(rng, k) for _ in range(4)] + [_pairs(rng, j) for j in range(7, k, 8)]
    return out + [_pairs(rng, k - 1) + "aa", _pairs(rng, k - 1) + "bb", _pairs(rng, k)[:-1], _pairs(rng, k - 1) + "a", "a" + _pairs(rng, k - 1) + "b"]


def _mix_members(k, rng):
    out = []
    for lead in (0, 1, 5):
        for j in (0, 1, k - 1, k, k + 1):
            for opt in ("", "d", "e"):
                out.append("c" * lead + _pairs(rng, j) + opt + "f")
    out += ["c" * 40 + _pairs(rng, k) + "df", "c" + _pairs(rng, k), _pairs(rng, k) + "d", _pairs(rng, k) + "ddf", _pairs(rng, k) + "dff",
            _pairs(rng, k - 1) + "aaf", _pairs(rng, k - 1) + "acf", _pairs(rng, k // 2) + "c" + _pairs(rng, k // 2) + "f", "f", "cf", "cdf"]
    return out + [_pairs(rng, j) + "ef" for j in range(7, k, 8)]


def _mix2_members(k, rng):
    out = []
    for j in (0, 1, k - 1, k, k + 1):
        for opt in ("", "c"):
            out += [_pairs(rng, j) + opt + "d", "ab" * j + opt + "d", "ba" * j + opt + "d"]
    out += [_pairs(rng, k), _pairs(rng, k) + "c", _pairs(rng, k) + "ccd", _pairs(rng, k) + "cdd", _pairs(rng, k - 1) + "aad", _pairs(rng, k - 1) + "acd", "d", "cd"]
    return out + [_pairs(rng, j) + "cd" for j in range(7, k, 8)]


def _carry3_like(n, rng, L):
    s = list(_ab(rng, L))
    if L > n:
        s[L - n - 1] = "a"
    return "".join(s)


FAMILIES = {
    # name: (shape, pattern, positions, alphabet, lengths around the accept edges, members, a likely member of about L bytes)
    "chain": ("chain", "a{1,%d}", lambda n: n + 1, "ab", lambda n: (0, 1, n - 1, n, n + 1, n + 2), _chain_members, lambda n, rng, L: "a" * L),
    "self": ("self", "a{%d}b*", lambda n: n + 2, "ab", lambda n: (n - 1, n, n + 1, n + 2, n + 40), _self_members,
             lambda n, rng, L: "a" * min(L, n) + "b" * max(L - n, 0)),
    "self2": ("self", "b+a{1,%d}", lambda n: n + 2, "ab", lambda n: (1, 2, n, n + 1, n + 2, n + 3), _self2_members,
              lambda n, rng, L: ("b" * rng.randint(1, 3) + "a" * L)[:max(L, 2)]),
    "carry": ("carry", "(a?){%d}b", lambda n: n + 2, "ab", lambda n: (0, 1, 2, n, n + 1, n + 2), _carry_members, lambda n, rng, L: "a" * max(L - 1, 0) + "b"),
    "carry2": ("carry", "b*a{1,%d}", lambda n: n + 2, "ab", lambda n: (0, 1, n - 1, n, n + 1, n + 2), _carry2_members,
               lambda n, rng, L: ("b" * rng.randint(0, 3) + "a" * L)[:max(L, 1)]),
    "carry3": ("carry", "(a|b)*a(a|b){%d}", lambda n: n + 3, "ab", lambda n: (n, n + 1, n + 2, n + 51), _carry3_members, _carry3_like),
    "exc": ("exc", "(ab|ba){1,%d}", lambda k: 4 * k + 2, "ab", lambda k: (0, 2, 3, 2 * k - 2, 2 * k, 2 * k + 1, 2 * k + 2), _exc_members,
            lambda k, rng, L: _pairs(rng, L // 2)),
    "mix": ("mix", "c*(ab|ba){1,%d}(d|e)?f", lambda k: 4 * k + 5, "abcdef", lambda k: (1, 3, 2 * k, 2 * k + 1, 2 * k + 2, 2 * k + 3, 2 * k + 4), _mix_members,
            lambda k, rng, L: "c" * rng.choice((0, 0, 1, 4)) + _pairs(rng, max(L - 2, 0) // 2) + rng.choice(("", "d", "e")) + "f"),
    "mix2": ("mix", "(ab|ba){1,%d}c?d", lambda k: 4 * k + 4, "abcd", lambda k: (1, 3, 2 * k, 2 * k + 1, 2 * k + 2, 2 * k + 3), _mix2_members,
             lambda k, rng, L: _pairs(rng, max(L - 2, 0) // 2) + rng.choice(("", "c")) + "d"),
}


def _table():
    rows = []                                              # (family, tag, n)
    for W in range(1, 17):
        rows.append(("chain", "", 32 * W - 1 if W in EDGE_WIDTHS else 32 * (W - 1) + 16))
        rows.append(("self", "", 32 * (W - 1) + 13))
        rows.append(("carry", "", 32 * (W - 1) + 20))      # one run of n + 1 positions: it straddles every word boundary of the program
        rows.append(("exc", "", 8 * W - 1))
        rows.append(("mix", "", 8 * W - 2))
    for W in EDGE_WIDTHS[1:]:                              # (a program of one word has no top word with bit 0 alone: a{1,n} has n + 1 >= 2 positions)
        rows.append(("chain", "bit0", 32 * (W - 1)))
    rows += [("self2", "", n) for n in (62, 169, 382, 510)]                   # 2, 6, 12 and 16 words (64, 384 and 512 positions: full top words)
    rows += [("carry2", "", n) for n in (70, 200, 300, 510)]                  # 3, 7, 10 and 16 words
    rows += [("carry3", "", n) for n in (40, 128, 270, 430)]                  # 2, 5, 9 and 14 words
    rows += [("mix2", "", k) for k in (31, 44, 100, 127)]                     # 4, 6, 13 and 16 words (128 and 512 positions: full top words)
    out = []
    for family, tag, n in rows:
        shape, pattern, positions, alphabet, lengths, _, _ = FAMILIES[family]
        nbits = positions(n)
        W = (nbits + 31) // 32
        out.append(Case("%s%s-W%d-n%d" % (family, "-" + tag if tag else "", W, n), shape, family, pattern % n, alphabet, W, nbits, n,
                        tuple(L for L in lengths(n) if L >= 0)))
    return out


CASES = _table()
RANDOM_LINES = 1500                                        # of 0 ... 130 bytes
MAX_CORPUS_BYTES = 300 << 10

_lines, _expected, _golden = {}, {}, None


def _mutate(rng, t, alphabet):
    """one byte replaced or removed, in the last forty bytes half of the time (where a long line's set sits in the top words)"""
    if not t:
        return rng.choice(alphabet)
    i = rng.randrange(max(len(t) - 40, 0), len(t)) if rng.random() < 0.5 else rng.randrange(len(t))
    return t[:i] + (rng.choice(alphabet.replace(t[i], "")) if rng.random() < 0.7 else "") + t[i + 1:]


def lines(case):
    """The lines of a case (bytes objects, no '\\n' inside), the same on every call: members of the language and near misses around
    every accept edge and every word boundary, one-letter and alternating lines of the edge lengths, mutants (among them the near
    misses that die in the top word), likely members around the edge lengths, RANDOM_LINES random lines of 0 ... 130 bytes, a line
    with a 0x00 byte and one with a byte >= 0x80."""
    if case.id in _lines:
        return _lines[case.id]
    rng = random.Random(case.id)
    _, _, _, alphabet, _, members, like = FAMILIES[case.family]
    out = [t for t in members(case.n, rng) if t is not None]
    a, b = alphabet[0], alphabet[1]
    for L in case.lengths:
        out += [c * L for c in alphabet[:3]] + [((a + b) * L)[:L], ((b + a) * L)[:L]]
    out += [_mutate(rng, t, alphabet) for t in list(out) if t]
    for _ in range(120):                                   # likely members around the edge lengths, a third of them with one byte wrong
        L = max(rng.choice(case.lengths) + rng.randint(-3, 3), 0)
        t = like(case.n, rng, L)
        out.append(_mutate(rng, t, alphabet) if rng.random() < 0.33 else t)
    for k in range(RANDOM_LINES):
        L = rng.randint(0, 130)
        if k % 2:
            out.append("".join(rng.choice(alphabet) for _ in range(L)))
        else:
            t = like(case.n, rng, L)
            out.append(_mutate(rng, t, alphabet) if rng.random() < 0.3 else t)
    rng.shuffle(out)
    out.sort(key=lambda t: t == "")                        # (stable: the empty lines last, then one that is not - without a final
    out.append(out.pop(0))                                 # newline an empty last line would be no line at all)
    out = [t.encode() for t in out]
    longest = max((t for t in members(case.n, random.Random(1)) if t), key=len).encode()
    mid = len(longest) // 2
    out.insert(len(out) // 3, longest[:mid] + b"\x00" + longest[mid:])
    out.insert(2 * len(out) // 3, longest[:mid] + b"\xc3\xa9" + longest[mid:])
    _lines[case.id] = out
    return out


def corpus(case, final_newline=True):
    return b"\n".join(lines(case)) + (b"\n" if final_newline else b"")


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nfa_width_vectors.json")
# The reference expands a{1,n} and (a?){n} into n * n / 2 edges and the oracle walks them byte by byte (b+a{1,n}, b*a{1,n} likewise): 100 us per byte at sixteen
# words, twenty seconds for one such corpus.  So the oracle's verdicts are RECORDED (tests/golden/make_nfa_width_vectors.py writes
# them, with a digest of the corpus they belong to), and the lowering test holds the record against the live oracle: on every line
# where that takes a moment, on a sample of the lines (the edge lengths among them) for the wide programs of these families.
SLOW_ORACLE = ("chain", "self2", "carry", "carry2")


def oracle_vector(case, indices=None):
    """The live oracle's verdict for the lines `indices` of the case (all of them: None), numpy uint8"""
    import numpy as np
    from pyoracle import OracleRegex
    o = OracleRegex(case.pattern)
    ls = lines(case)
    return np.array([1 if o.accepts(ls[i]) else 0 for i in (range(len(ls)) if indices is None else indices)], dtype=np.uint8)


def oracle_sample(case):
    """indices of the lines the lowering test asks the live oracle about: None = all of them"""
    if case.family not in SLOW_ORACLE or case.W <= 4:
        return None
    return sorted(set(range(0, len(lines(case)), 7)) | set(edge_lines(case)[:8]))


def digest(case):
    return hashlib.sha1(corpus(case)).hexdigest()


def expected(case):
    """The oracle's verdict per line (numpy uint8, read-only), as recorded for exactly this corpus"""
    global _golden
    if case.id not in _expected:
        import numpy as np
        if _golden is None:
            with open(GOLDEN) as f:
                _golden = json.load(f)
        g = _golden.get(case.id)
        assert g is not None and g["sha1"] == digest(case), "%s: the case table changed - run tests/golden/make_nfa_width_vectors.py" % case.id
        n = len(lines(case))
        v = np.unpackbits(np.frombuffer(bytes.fromhex(g["bits"]), dtype=np.uint8), bitorder="little")[:n].copy()
        assert g["lines"] == n
        v.setflags(write=False)
        _expected[case.id] = v
    return _expected[case.id]


def edge_lines(case):
    """indices of the lines of the edge lengths (the facade runs one string per call: a few dozen of them)"""
    want = set(case.lengths)
    idx = [i for i, t in enumerate(lines(case)) if len(t) in want]
    return idx[:40]


# ---- the sampled table's recheck kernels (recheck_lines_kernel<W>, recheck_escaped_kernel<W>: PlainNfaEngine<W>) at more than one width.
# [a-c]{1,6}:(x|y)*x(x|y){n} does not determinise (2^(n+1) sets on x/y text), AUTO leaves it on the NFA lane engine, and a table learnt
# from lines that hold the prefix and at most two bytes of x/y has thirty states: every longer x/y tail ESCAPES and is decided by the
# NFA engine.  (n, program width): a padded and an exact program for the six-word kernels, the exact twelve, a padded sixteen.  A table
# is learnt at every width tried (two to sixteen words): none is left out because it could not be.
SAMPLED_CASES = ((140, 5), (170, 6), (360, 12), (420, 14))
SAMPLED_LIST_FLOOR = 1024            # corpus.cpp, match_corpus_sampled: `cap = std::max<size_t>(words / 2, 1024)` listed escaped lines, words =
                                     # bitmap words of the corpus (lines / 32); more escapes than that: the walk over the stripes
SAMPLED_RETIRE_PERCENT = 5           # sampled.hpp: kRetireEscapePercent - a launch above it retires the table (the next one is the NFA engine's)


def sampled_pattern(n):
    return "[a-c]{1,6}:(x|y)*x(x|y){%d}" % n


def sampled_list_capacity(nlines):
    return max(((nlines + 31) // 32) // 2, SAMPLED_LIST_FLOOR)


def _like_sample(rng):
    t = "".join(rng.choice("abc") for _ in range(rng.randint(1, 6))) + ":"
    k = rng.random()
    return t + rng.choice(("x", "y", "xy", "yx")) if k < 0.1 else t[:-1] if k < 0.2 else t


def sampled_sample():
    """the text the table is learnt from: 2000 lines"""
    rng = random.Random(3)
    return ("\n".join(_like_sample(rng) for _ in range(2000)) + "\n").encode()


def _escaping(rng, n, accept, length=None):
    """a line with an x/y tail of n bytes or more (the table decides the short ones: it rejects them); accept: an x stands n + 1 bytes
    from the end"""
    L = length if length is not None else rng.choice((n, n + 1, n + 2, n + 30, n + 61))
    if accept:
        L = max(L, n + 1)
    s = [rng.choice("xy") for _ in range(L)]
    if L > n:
        s[L - n - 1] = "x" if accept else "y"
    return "".join(rng.choice("abc") for _ in range(rng.randint(1, 6))) + ":" + "".join(s)


def sampled_few(n, stripe):
    """-> (corpus bytes, final '\\n' included; indices of the escaping lines; index of the one that starts at a multiple of `stripe`): a
    dozen escaping lines among three thousand - the first and the last line, one at a stripe boundary, one longer than a stripe"""
    rng = random.Random(n * 7 + stripe)
    out, esc = [_escaping(rng, n, True)], [0]
    out += [_like_sample(rng) for _ in range(700)]
    gap = -sum(len(t) + 1 for t in out) % stripe
    if gap in (1, 2):
        gap += stripe
    while gap:                                             # filler lines of 3 ... 8 bytes with their '\n'
        k = gap if gap <= 8 else 6 if gap - 8 in (1, 2) else 8
        out.append("abc"[gap % 3] * (k - 2) + ":")
        gap -= k
    boundary = len(out)
    esc.append(boundary)
    out.append(_escaping(rng, n, True, n + 1))
    out += [_like_sample(rng) for _ in range(700)]
    esc.append(len(out))
    out.append(_escaping(rng, n, True, stripe + n + 77))   # longer than a stripe
    for k in range(8):
        out += [_like_sample(rng) for _ in range(200)]
        esc.append(len(out))
        out.append(_escaping(rng, n, k % 2 == 0))
    out += [_like_sample(rng) for _ in range(50)]
    esc.append(len(out))
    out.append(_escaping(rng, n, False, stripe + 5))
    esc.append(len(out))
    out.append(_escaping(rng, n, True))
    return ("\n".join(out) + "\n").encode(), esc, boundary


def sampled_many(n):
    """-> (corpus bytes; indices of the escaping lines): more escaping lines than the list holds, fewer than retire the table"""
    rng = random.Random(n * 11)
    out, esc = [], []
    for i in range(24000):
        if i % 22 == 0 or i == 23999:
            esc.append(i)
            out.append(_escaping(rng, n, rng.random() < 0.5))
        else:
            out.append(_like_sample(rng))
    return ("\n".join(out) + "\n").encode(), esc
