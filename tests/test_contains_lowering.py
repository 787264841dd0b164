"""The contains table (rrx_contains_corpus) on the CPU: RRX_PROGRAM_CONTAINS_DFA and its stride-2 form are replayed line by line
(start state at a line start, verdict of the state at the line end) and compared with two independent oracles - the brute-force
search on short lines with NUL and high bytes, the oracle's own automaton of .*(p).* on long ASCII lines."""
import random
import time

import numpy as np

import roaringregex_amd as rr
from contains_cases import (EXPLODING, alphabet_for, brute_force, dot_star, long_ascii_lines, short_line_patterns, short_lines,
                            split_lines)
from patterns import EMAIL, K1000_CONTAINS, U2
from program_replay import Dfa2Replay, DfaReplay

TABLE_ENGINES = ("dfa-stride2-table", "dfa-wide-table", "dfa-classed-table", "dfa-global-table")


def replay_dfa(words, lines):
    """DfaReplay's arrays stepped in contains mode: class 0 (NUL, >= 0x80) is an ordinary column, nothing rejects."""
    d = DfaReplay(words)
    out = []
    for ln in lines:
        st = d.start
        for c in ln:
            st = int(d.next[st, d.cls[c]])
        out.append(int(d.acc[st]))
    return np.array(out, dtype=np.uint8)


def replay_dfa2(words, data):
    """Dfa2Replay over the text as the kernel steps it: bytes >= 0x80 as 0x00 (the same class; they cannot index the pair table)."""
    a = np.frombuffer(bytes(data), dtype=np.uint8).copy()
    a[a >= 0x80] = 0
    return np.array(Dfa2Replay(words).match_lines(a.tobytes()), dtype=np.uint8)


def check(p, data, want, r=None):
    r = r or rr.RRegex(p)
    lines = split_lines(data)
    assert len(want) == len(lines)
    words = r.program(rr.PROGRAM_CONTAINS_DFA)
    assert words is not None, (p[:40], "no contains table")
    got = replay_dfa(words, lines)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (p[:40], "DFA", int(bad[0]), lines[bad[0]], int(got[bad[0]]))
    w2 = r.program(rr.PROGRAM_CONTAINS_DFA2)
    if r.contains_engine_name == "dfa-stride2-table":
        assert w2 is not None
    if w2 is not None:
        got2 = replay_dfa2(w2, data)
        assert got2.shape == got.shape and (got2 == got).all(), (p[:40], "the two program kinds disagree", int(np.nonzero(got2 != got)[0][0]))
    return r


def check_table(p, r):
    fwd = r.program(rr.PROGRAM_SEARCH_FWD)
    assert fwd is not None, (p[:40], "no forward search table")
    assert 1 <= r.contains_states <= int(fwd[0]) + 1, (p[:40], r.contains_states, int(fwd[0]))
    assert r.contains_engine_name in TABLE_ENGINES, p[:40]
    words = r.program(rr.PROGRAM_CONTAINS_DFA)
    d = DfaReplay(words)
    assert d.nstates == r.contains_states
    assert not d.acc[0] and (d.next[0] == 0).all(), (p[:40], "state 0 is not an absorbing rejecting SKIP row")
    if d.start != 0:                                   # (the empty language: SKIP is the start) - else nothing leads to SKIP
        assert (d.next[1:] != 0).all(), (p[:40], "SKIP is reachable")


def test_contains_tables_on_short_lines_with_nul_and_high_bytes():
    rng = random.Random(771)
    pats = short_line_patterns() + ["a*"]
    for p in pats:
        r = rr.RRegex(p)
        check_table(p, r)                              # (no pattern of this set may be unsupported: contains_engine_name raises)
        lines = short_lines(rng, p, 400)
        for tail in (b"\n", b""):
            data = b"\n".join(lines) + tail
            check(p, data, brute_force(p, data), r)


def test_contains_tables_on_long_ascii_lines():
    rng = random.Random(772)
    for p in short_line_patterns()[:20] + [EMAIL, U2, "a*"]:
        lines = long_ascii_lines(rng, p, 24)
        check(p, b"\n".join(lines) + b"\n", dot_star(p, lines))


def test_contains_table_of_the_keyword_set():
    p = K1000_CONTAINS
    r = rr.RRegex(p)
    check_table(p, r)
    rng = random.Random(773)
    words = ["k%d" % rng.randrange(3000) for _ in range(40)]
    lines = [(" ".join(rng.choice(words + ["x", "kk", "k", "10"]) for _ in range(rng.randint(0, 12)))).encode() for _ in range(150)]
    lines += long_ascii_lines(rng, p, 6, maxlen=1500)
    check(p, b"\n".join(lines), dot_star(p, lines), r)


def test_nullable_and_degenerate():
    r = rr.RRegex("a*")
    assert r.contains_states == 2                      # SKIP and FOUND
    for data in (b"\n", b"\n\n\n", b"b", b"\xff\n\x00"):
        check("a*", data, np.ones(len(split_lines(data)), dtype=np.uint8), r)
    check("ab", b"", np.zeros(0, dtype=np.uint8))
    # the empty language is contained in nothing: SKIP is the whole table
    r = rr.RRegex("[]")
    assert r.contains_states == 1
    check("[]", b"\nab\n\xff", np.zeros(3, dtype=np.uint8), r)
    # high bytes do not reject: the reason the entry exists
    check(U2, b"caf\xc3\xa9 http://a.bc\nna\xc3\xafve\n\x00ftp://x.yz/z\n", np.array([1, 0, 1], dtype=np.uint8))


def test_exploding_subset_construction_is_reported_not_hung():
    r = rr.RRegex(EXPLODING)
    t0 = time.time()
    fwd = r.program(rr.PROGRAM_SEARCH_FWD)             # build_search: the budget the contains build is bounded by
    t_search = time.time() - t0
    r2 = rr.RRegex(EXPLODING)
    t0 = time.time()
    assert r2.contains_states == 0
    t_contains = time.time() - t0
    assert fwd is None
    assert rr._L.rrx_contains_engine_name(r2._h) is None
    msg = rr._L.rrx_last_error().decode()
    assert "contains" in msg and "determinise" in msg, msg
    try:
        r2.contains_engine_name
        raise AssertionError("expected RRegexError")
    except rr.RRegexError:
        pass
    assert r2.program(rr.PROGRAM_CONTAINS_DFA) is None and r2.program(rr.PROGRAM_CONTAINS_DFA2) is None
    assert t_contains <= 2 * t_search + 1.0, (t_contains, t_search)      # the same construction, the same budget (timer noise allowed for)


def test_forced_table_forms():
    """RRX_ENGINE_DFA keeps the contains table on the byte-stride LDS form, RRX_ENGINE_DFA_GLOBAL on the global one; the table is the same."""
    for p in (U2, EMAIL, "ab+c"):
        names = {}
        for e in (rr.ENGINE_AUTO, rr.ENGINE_DFA, rr.ENGINE_DFA_GLOBAL):
            r = rr.RRegex(p, e)
            names[e] = r.contains_engine_name
            assert (r.program(rr.PROGRAM_CONTAINS_DFA) == rr.RRegex(p).program(rr.PROGRAM_CONTAINS_DFA)).all()
        # (U2's contains table has 364 states of 16 classes: its stride-2 form passes the LDS region, AUTO keeps it on the classed table)
        assert names[rr.ENGINE_AUTO] == ("dfa-classed-table" if p == U2 else "dfa-stride2-table"), (p, names)
        assert names[rr.ENGINE_DFA] in ("dfa-wide-table", "dfa-classed-table"), (p, names)
        assert names[rr.ENGINE_DFA_GLOBAL] == "dfa-global-table", (p, names)
