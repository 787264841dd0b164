"""The automata that sit ON the limit of a table form, and their first neighbours beyond it - the case set of
test_table_edges_lowering.py (CPU) and test_table_edges_gpu.py (device).  Plain data and the builders of the texts; no device call.

Every table engine packs "next row" into a narrow field, and the planner admits an automaton by a `<=` against a constant chosen so
that the largest offset just fits (csrc/plan.cpp, device.hpp, pack.cpp):

    wide byte-stride       nstates <= 127; R = 1 ... 32 interleaved copies while nstates * 516 * R <= 65536 (16-bit row byte offsets)
    classed byte-stride    nstates * (ncls + 2) <= 16384 (16-bit row byte offsets of 4-byte entries)
    stride-2               nstates * (ncols | 1) * 4 <= 43008 (16-bit LDS address of the next row; 1024 window words left at the limit)
    byte-stride items      nstates * 131 * 4 * R <= 65535 (125 states)
    stride-2 items         as stride-2, on the items form (one code more)
    plain tables           PlainDfaEngine::lds_bytes of one table, or of two together, <= 65536, else HBM/L2 (a{13054}: 65536 to the
                           byte, no contains table; the literal of 511 letters and digits: the largest whose match AND contains table fit)

A case names its pattern, the engine to request, the table it is about (match / contains / items / plain), the form the library
must choose, the limit and the side of it.  `a{n}` lowers to n + 2 states (row 0 dead, row 1 the start, row n + 1 accepting and the
row at the highest offset), 2 byte classes and 7 pair columns; `(ab|cd|ef){n}` to 4 n + 2 states and 20 pair columns (even: the pad
column is in use); the 62 letters and digits as one literal, k times, to 62 k + 2 states of 63 classes.

THE TEXT RULE (build_lines): for every member - a line that walks through every row, for a{n} the n a's - the text holds the member,
the member one byte short and one byte long, and the member with its last byte changed to another byte of the alphabet, to NUL and
to 0xC3 (column 128 / class 0 from the highest row); empty lines and every one-byte line.  These lines repeat in rounds of an odd
number of bytes (so that every line meets both pair alignments and many stripe offsets) until the text passes a workgroup's
512 KiB at stripe 512 by 64 KiB; the first member is placed across the workgroup cut.

EXPECTED VALUES (expected): OracleRegex.match_lines over the whole text, cross-checked line by line against Python's re (the
patterns here mean the same in both dialects).  Two exceptions, which rest on the closed form (re.fullmatch: 1 <= len <= n and all
bytes 'a') ALONE for their long lines: a{1,1534} and a{1,1535} - the oracle needs about 1.3 s per line of 1534 a's - where the
oracle checks every distinct line shorter than 64 bytes and two long ones (the member and the member one byte long); all other
lines of these two cases (the member one byte short and its three changed-last-byte forms) are covered by the closed form only.
Contains cases: re.search per line (bytes >= 0x80 and NUL are ordinary text that no pattern here matches), cross-checked on every
distinct line without such bytes against the oracle's own automaton of .*(p).*."""
import functools
import re
from typing import NamedTuple

import numpy as np

import roaringregex_amd as rr

ALNUM = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789"
WG_STRIPES = 1024                          # stripes per workgroup of the batch kernels
WG_BYTES = WG_STRIPES * 512                # a workgroup's text at stripe 512
TEXT_BYTES = WG_BYTES + (64 << 10)
DFA2_WINDOW_WORDS_AT_LIMIT = 1024          # dfa2_window_words of a 43008-byte table: (46 KiB - 43008) / 4

WIDE_MAX_STATES, CLASSED_MAX_ENTRIES, DFA2_MAX_TABLE, PLAIN_LDS_BUDGET = 127, 16384, 43008, 65536


class Case(NamedTuple):
    id: str
    pattern: str
    engine: int            # the engine to request
    table: str             # match | contains | items | plain | plain2
    form: str              # the form the library must report (engine_name / contains_engine_name), or the path for items / plain
    limit: str             # the fit expression
    side: str              # "at": the largest of its family that fits; "past": the first that does not; "inside"
    value: int             # what the fit expression must evaluate to
    members: tuple         # lines that together walk through every row
    closed_form: bool = False


def _a(n):
    return (b"a" * n,)


def _alt(n):
    return (b"ab" * n, b"cd" * n, b"ef" * n)


def _lit(k):
    return ((ALNUM * k).encode(),)


def _cases():
    D, A = rr.ENGINE_DFA, rr.ENGINE_AUTO
    out = []
    # ---- wide form: the state limit, and both sides of every copy-count step (R = 32|16 at 3|4 states ... 2|1 at 63|64)
    for n, copies, side in ((1, 32, "at"), (2, 16, "past"), (5, 16, "at"), (6, 8, "past"), (13, 8, "at"), (14, 4, "past"), (29, 4, "at"), (30, 2, "past"),
                            (61, 2, "at"), (62, 1, "past")):
        out.append(Case("wide-copies-a{%d}" % n, "a{%d}" % n, D, "match", "dfa-wide-table", "nstates * 516 * R <= 65536, R = %d" % copies, side,
                        (n + 2) * 516 * copies, _a(n)))
    out.append(Case("wide-a{125}", "a{125}", D, "match", "dfa-wide-table", "nstates <= 127", "at", 127, _a(125)))
    out.append(Case("wide-past-a{126}", "a{126}", D, "match", "dfa-classed-table", "nstates <= 127", "past", 128, _a(126)))
    # ---- classed form
    out.append(Case("classed-a{4094}", "a{4094}", D, "match", "dfa-classed-table", "nstates * (ncls + 2) <= 16384", "at", 16384, _a(4094)))
    out.append(Case("classed-past-a{4095}", "a{4095}", D, "match", "dfa-global-table", "nstates * (ncls + 2) <= 16384", "past", 16388, _a(4095)))
    out.append(Case("classed-alnum-x4", ALNUM * 4, D, "match", "dfa-classed-table", "nstates * (ncls + 2) <= 16384", "at", 250 * 65, _lit(4)))
    out.append(Case("classed-past-alnum-x5", ALNUM * 5, D, "match", "dfa-global-table", "nstates * (ncls + 2) <= 16384", "past", 312 * 65, _lit(5)))
    # ---- stride-2 form
    s2 = "nstates * (ncols | 1) * 4 <= 43008"
    out.append(Case("stride2-a{1534}", "a{1534}", A, "match", "dfa-stride2-table", s2, "at", 43008, _a(1534)))
    out.append(Case("stride2-past-a{1535}", "a{1535}", A, "match", "dfa-classed-table", s2, "past", 43036, _a(1535)))
    out.append(Case("stride2-a{1,1534}", "a{1,1534}", A, "match", "dfa-stride2-table", s2, "at", 43008, _a(1534), True))
    out.append(Case("stride2-past-a{1,1535}", "a{1,1535}", A, "match", "dfa-classed-table", s2, "past", 43036, _a(1535), True))
    out.append(Case("stride2-alt{127}", "(ab|cd|ef){127}", A, "match", "dfa-stride2-table", s2, "at", 510 * 21 * 4, _alt(127)))
    out.append(Case("stride2-past-alt{128}", "(ab|cd|ef){128}", A, "match", "dfa-classed-table", s2, "past", 514 * 21 * 4, _alt(128)))
    out.append(Case("stride2-alnum-x2", ALNUM * 2, A, "match", "dfa-stride2-table", s2, "inside", 126 * 69 * 4, _lit(2)))
    out.append(Case("stride2-past-alnum-x3", ALNUM * 3, A, "match", "dfa-classed-table", s2, "past", 188 * 69 * 4, _lit(3)))
    # ---- contains tables: separate LineTables with the same rules (8 pair columns for a{n}: one more than the match table)
    out.append(Case("contains-wide-a{125}", "a{125}", D, "contains", "dfa-wide-table", "nstates <= 127", "at", 127, _a(125)))
    out.append(Case("contains-wide-past-a{126}", "a{126}", D, "contains", "dfa-classed-table", "nstates <= 127", "past", 128, _a(126)))
    out.append(Case("contains-classed-a{4094}", "a{4094}", A, "contains", "dfa-classed-table", "nstates * (ncls + 2) <= 16384", "at", 16384, _a(4094)))
    out.append(Case("contains-classed-past-a{4095}", "a{4095}", A, "contains", "dfa-global-table", "nstates * (ncls + 2) <= 16384", "past", 16388, _a(4095)))
    out.append(Case("contains-stride2-a{1192}", "a{1192}", A, "contains", "dfa-stride2-table", s2, "at", 1194 * 9 * 4, _a(1192)))
    out.append(Case("contains-stride2-past-a{1193}", "a{1193}", A, "contains", "dfa-classed-table", s2, "past", 1195 * 9 * 4, _a(1193)))
    # ---- items tables (explicit items with a separator byte each)
    i1 = "nstates * 131 * 4 * R <= 65535"
    out.append(Case("items-a{123}", "a{123}", A, "items", "byte-stride items table", i1, "at", 125 * 524, _a(123)))
    out.append(Case("items-past-a{124}", "a{124}", A, "items", "lane per item", i1, "past", 126 * 524, _a(124)))
    out.append(Case("items2-a{1534}", "a{1534}", A, "items", "stride-2 items table", s2, "at", 43008, _a(1534)))
    out.append(Case("items2-past-a{1535}", "a{1535}", A, "items", "lane per item", s2, "past", 43036, _a(1535)))
    # ---- plain tables of the lane-per-item kernels
    out.append(Case("plain-a{13054}", "a{13054}", A, "plain", "lds", "plain_lds_bytes(table) <= 65536", "at", 65536, _a(13054)))
    out.append(Case("plain-past-a{13055}", "a{13055}", A, "plain", "global", "plain_lds_bytes(table) <= 65536", "past", 65568, _a(13055)))
    # (a{n} beyond 6500 states has no contains table: the literal of 511 letters and digits - 513 states of 63 classes - is the largest
    # of its family whose match table AND contains table stay in LDS)
    lit = (ALNUM * 9)[:512]
    out.append(Case("plain-literal-511", lit[:511], D, "plain", "lds", "plain_lds_bytes(table) <= 65536", "at", 65424, (lit[:511].encode(),)))
    out.append(Case("plain-past-literal-512", lit, D, "plain", "global", "plain_lds_bytes(table) <= 65536", "past", 65552, (lit.encode(),)))
    out.append(Case("plain2-a{6498}", "a{6498}", A, "plain2", "lds", "plain_lds_bytes(starts) + plain_lds_bytes(anchored) <= 65536", "at", 65536, _a(6498)))
    out.append(Case("plain2-past-a{6499}", "a{6499}", A, "plain2", "global", "plain_lds_bytes(starts) + plain_lds_bytes(anchored) <= 65536", "past", 65568,
                    _a(6499)))
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
# the first pattern of each stride-2 family that no longer fits: RRX_ENGINE_DFA2 must refuse it
DFA2_REFUSED = [c.pattern for c in CASES if c.table == "match" and c.side == "past" and c.id.startswith("stride2-")]


def cases(table, side=None):
    return [c for c in CASES if c.table == table and (side is None or c.side == side)]


# ---------------------------------------------------------------------------------------------- the fit rules, restated
def plain_table_bytes(words):
    """LDS bytes of a plain table (PlainDfaEngine): next, the byte -> class map, the accept flags."""
    nstates, ncls = int(words[0]), int(words[1])
    return nstates * ncls * 2 + 256 + nstates


def plain_lds_bytes(words):
    """PlainDfaEngine::lds_bytes to the byte - what the kernels compare with the 64 KiB budget: the two arrays rounded up to 16."""
    nstates, ncls = int(words[0]), int(words[1])
    return ((nstates * ncls * 2 + 15) & ~15) + 256 + ((nstates + 15) & ~15)


def wide_copies(nstates):
    """pack.cpp: the interleaved copies of a wide line table."""
    rep = 0
    while rep < 5 and nstates * 129 * 4 * (2 << rep) <= 65536:
        rep += 1
    return 1 << rep


def items_copies(nstates):
    """pack.cpp: the interleaved copies of a byte-stride items table."""
    rep = 0
    while rep < 3 and nstates * 131 * 4 * (2 << rep) <= 60 * 1024:
        rep += 1
    return 1 << rep


def dfa2_copies(nstates, ncols):
    """pack.cpp: dfa2_copies_log2."""
    rep = 0
    while rep < 5 and nstates * (ncols | 1) * 4 * (2 << rep) <= 30 * 1024 and ncols * 4 * (2 << rep) <= 65535:
        rep += 1
    return 1 << rep


def dfa2_bytes(words):
    return int(words[0]) * (int(words[1]) | 1) * 4


def classed_entries(words):
    return int(words[0]) * (int(words[1]) + 2)


# ---------------------------------------------------------------------------------------------- texts
def other_byte(case, member):
    """Another byte of the pattern's alphabet than the member's last (a pattern of one letter: 'b')."""
    letters = sorted(set(b"".join(case.members)))
    for c in letters:
        if c != member[-1]:
            return bytes([c])
    return b"b"


def distinct_lines(case, high=True):
    """The lines the text rule asks for, each once: empty, one byte, and the six forms of every member."""
    one = sorted(set(b"".join(case.members)) | {ord("b")})
    lines = [b""] + [bytes([c]) for c in one] + [b"\x00"] + ([b"\xc3"] if high else [])
    for m in case.members:
        lines += [m, m[:-1], m + m[-1:], m[:-1] + other_byte(case, m), m[:-1] + b"\x00"] + ([m[:-1] + b"\xc3"] if high else [])
        if case.table in ("contains", "plain", "plain2"):            # a match behind text that went part of the way, and in the middle of a line
            lines += [m[:-1] + other_byte(case, m) + m, b"b" + m + b"b", b"\xc3" + m if high else b"\x00" + m]
    seen, out = set(), []
    for ln in lines:
        if ln not in seen:
            seen.add(ln)
            out.append(ln)
    return out


@functools.lru_cache(maxsize=4)
def build_lines(case_id, high=True, total=TEXT_BYTES):
    """The text of a case as (distinct lines, index of the distinct line per text line): rounds of an odd number of bytes, the
    first member across the workgroup cut, `total` bytes at least."""
    case = BY_ID[case_id]
    distinct = distinct_lines(case, high)
    rnd = list(range(len(distinct)))
    if sum(len(distinct[i]) + 1 for i in rnd) % 2 == 0:
        rnd.append(0)                               # one more empty line: the round's length is odd
    rbytes = sum(len(distinct[i]) + 1 for i in rnd)
    first = distinct.index(case.members[0])
    one_byte = 1                                    # (distinct[1] is a one-byte line)
    assert len(distinct[one_byte]) == 1
    idx, at, cut_done = [], 0, total <= WG_BYTES
    while at < total:
        m = len(distinct[first])
        if not cut_done and at + rbytes > WG_BYTES - m:
            pad = WG_BYTES - (m + 1) // 2 - at      # the member begins (m + 1) / 2 bytes in front of the cut
            assert pad >= 0
            idx += [one_byte] * (pad // 2) + [0] * (pad % 2)
            at += pad
            if m >= 2:
                assert at < WG_BYTES < at + m
            cut_done = True
            idx.append(first)
            at += m + 1
            continue
        idx += rnd
        at += rbytes
    return distinct, np.array(idx, dtype=np.int64)


def text_of(distinct, idx):
    return np.frombuffer(b"".join(distinct[i] + b"\n" for i in idx), dtype=np.uint8).copy()


def line_starts(distinct, idx):
    lens = np.array([len(ln) + 1 for ln in distinct], dtype=np.int64)[idx]
    return np.concatenate([[0], np.cumsum(lens)[:-1]]), lens - 1


def closed_form(case, distinct):
    """uint8 per distinct line from Python's re: the whole line for the match and items tables, a substring for contains."""
    rx = re.compile(case.pattern.encode())
    if case.table == "contains":
        return np.array([1 if rx.search(ln) else 0 for ln in distinct], dtype=np.uint8)
    return np.array([1 if rx.fullmatch(ln) else 0 for ln in distinct], dtype=np.uint8)


def contains_expected(case, distinct):
    """uint8 per distinct line: re.search, cross-checked on every line without NUL and bytes >= 0x80 against the oracle's own
    automaton of .*(p).*."""
    from pyoracle import OracleRegex
    rx = re.compile(case.pattern.encode())
    per_line = np.array([1 if rx.search(ln) else 0 for ln in distinct], dtype=np.uint8)
    o = OracleRegex(".*(" + case.pattern + ").*")
    for ln, v in zip(distinct, per_line):
        if not any(c == 0 or c >= 0x80 for c in ln):
            assert bool(o.accepts(ln.decode("latin-1"))) == bool(v), (case.id, len(ln), int(v))
    return per_line


@functools.lru_cache(maxsize=None)
def _oracle_line(pattern, line):
    """The oracle's verdict on one line (kept: a long line of a{1,1534} costs it more than a second)."""
    from pyoracle import OracleRegex
    return int(OracleRegex(pattern).match_lines(np.frombuffer(line + b"\n", dtype=np.uint8))[0])


@functools.lru_cache(maxsize=8)
def expected(case_id, high=True, total=TEXT_BYTES):
    """(text uint8, expected verdict per line uint8): see the module docstring."""
    from pyoracle import OracleRegex
    case = BY_ID[case_id]
    distinct, idx = build_lines(case_id, high, total)
    per_line = closed_form(case, distinct)
    data, want = text_of(distinct, idx), per_line[idx]
    if case.table == "contains":
        assert (contains_expected(case, distinct) == per_line).all()
    elif case.closed_form:
        m = case.members[0]
        for ln, v in zip(distinct, per_line):
            if len(ln) < 64 or ln in (m, m + m[-1:]):
                assert _oracle_line(case.pattern, ln) == int(v), (case_id, len(ln), int(v))
    else:
        oracle = OracleRegex(case.pattern).match_lines(data)
        assert oracle.shape == want.shape and (oracle == want).all(), (case_id, "oracle and re disagree on line", int(np.nonzero(oracle != want)[0][0]))
    return data, want


def window_overflow_text(seed=5, nbytes=2 * WG_BYTES + 1000):
    """Lines of 1 to 3 bytes from {a, b} for a{1,1534}: a workgroup at stripe 512 ends more than 1024 * 32 lines, so its result
    words pass the 1024-word window the table leaves, with accepted bits beyond it.  -> (text, expected)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 4, size=nbytes // 2)
    ends = np.cumsum(lens + 1)                                   # one past each line's '\n'
    lens, ends = lens[ends <= nbytes + 4], ends[ends <= nbytes + 4]
    data = np.frombuffer(b"aaab", dtype=np.uint8)[rng.integers(0, 4, size=int(ends[-1]))].copy()
    data[ends - 1] = 10
    starts = ends - lens - 1
    a_count = np.add.reduceat((data == ord("a")).astype(np.int64), starts)
    return data, (a_count == lens).astype(np.uint8)
