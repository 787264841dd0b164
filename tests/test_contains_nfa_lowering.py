"""Contains on the NFA lane engine (RRX_OPT_CONTAINS_NFA) on the CPU: the option, the route and its error texts, the dump of the
program the kernels run (RRX_PROGRAM_CONTAINS_NFA), and a replay of that program - in the LINE form of ContainsLineNfaEngine and in
the PLAIN form of contains_extents_nfa_kernel (kernels_nfa.inc) - against the expectations of contains_nfa_cases.py, which
test_contains_nfa_gpu.py holds the kernels to.  No GPU needed.

The replay is LineNfaEngine's / NfaCore's step (program_replay.NfaReplay) with the three changes that make it contains:
  (a) position 0, the initial state, stays live on every byte (line form: position 0 in every B row; plain form: S |= init);
  (b) the rows of NUL and of bytes >= 0x80 are {position 0}, not empty (line form; the plain form's S |= init does not ask the row);
  (c) a sticky found |= S & FIN after every step, read and cleared at the line end (plain form: the walk ends at the first hit).
test_the_lines_are_sharp drops each of them, and clears the top word of S, and sees a verdict change in every case."""
import random
import re

import numpy as np
import pytest

import contains_cases as CC
import contains_nfa_cases as T
import nfa_width_cases as WC
import roaringregex_amd as rr
from program_replay import NfaReplay

_regexes, _replays = {}, {}
NEEDS_BOTH_REASONS = "(a|b)*a(a|b){600}"                  # no contains table (2^601 sets) and 603 positions: no lane program either


def regex(pattern):
    if pattern not in _regexes:
        _regexes[pattern] = rr.RRegex(pattern)
    return _regexes[pattern]


class ContainsNfaReplay(NfaReplay):
    """drop: '' or one of 'a', 'b', 'c' (the change left out), 'top' (the top word of S cleared after every step)"""

    def _step(self, S, row, line_form):
        t = ((S << 1) & self.mask) | 1 if line_form else (S << 1) & self.mask & self.chain
        t |= (S & self.self_) | (((S & self.cgrp) + self.cgrp) & self.ctgt)
        e = S & self.excm
        while e:
            b = (e & -e).bit_length() - 1
            e &= e - 1
            t |= self.X[b]
        return t & row

    def _keep(self, drop):
        return (1 << (32 * (self.W - 1))) - 1 if drop == "top" else self.mask

    def contains_lines(self, data, drop=""):
        """ContainsLineNfaEngine: no CHAIN mask, a 1 shifted into position 0, B['\\n'] = {position 0}; one verdict per line"""
        assert self.init == 1
        B = list(self.B)
        if drop == "a":
            B = [b & ~1 for b in B]
        if drop == "b":
            B = [0 if (c == 0 or c >= 0x80) else b for c, b in enumerate(B)]
        keep = self._keep(drop)
        seq = bytes(data)
        if seq and seq[-1] != 10:
            seq += b"\n"                          # end of data ends the last line
        out, S, found = [], self.init, 0
        for c in seq:
            if c == 10:
                out.append(1 if (S & self.fin if drop == "c" else found) else 0)
                found = 0
            S = self._step(S, 1 if c == 10 else B[c], True) & (keep | 1)
            found |= S & self.fin
        return np.array(out, dtype=np.uint8)

    def contains_item(self, item, drop=""):
        """contains_extents_nfa_kernel: NfaCore's step with the CHAIN mask, then S |= init; '\\n' an ordinary byte"""
        keep = self._keep(drop)
        S = self.init
        hit = (S & self.fin) != 0
        for c in bytes(item):
            if hit and drop != "c":
                break
            S = self._step(S, self.B[c], False) & keep
            if drop != "a":
                S |= self.init
            hit = (S & self.fin) != 0
        return 1 if hit else 0

    def contains_items(self, lines, drop=""):
        return np.array([self.contains_item(t, drop) for t in lines], dtype=np.uint8)


def replay(pattern):
    if pattern not in _replays:
        w = regex(pattern).program(rr.PROGRAM_CONTAINS_NFA)
        assert w is not None, pattern
        _replays[pattern] = ContainsNfaReplay(w)
    return _replays[pattern]


# ---- the option and the route
def test_option_values():
    r = rr.RRegex("ab+c")
    for mode in (0, 1, 2, 0):
        r.set_contains_nfa(mode)
    for bad in (3, -1):
        with pytest.raises(rr.RRegexError):
            r.set_contains_nfa(bad)
    assert rr.OPT_CONTAINS_NFA == 7 and rr.PROGRAM_CONTAINS_NFA == 25


def test_the_default_stays():
    r = rr.RRegex(CC.EXPLODING)
    assert r.contains_states == 0
    with pytest.raises(rr.RRegexError, match="determinise"):
        r.contains_engine_name


def test_engine_name_follows_the_route():
    r = rr.RRegex(CC.EXPLODING)
    r.set_contains_nfa(1)
    assert r.contains_engine_name == "nfa-shift-and" and r.contains_states == 0
    r.set_contains_nfa(0)
    with pytest.raises(rr.RRegexError, match="determinise"):
        r.contains_engine_name
    t = rr.RRegex("ab+c")                                  # a pattern with a table: option 1 keeps it, option 2 sets it aside
    table, states = t.contains_engine_name, t.contains_states
    assert table.startswith("dfa-") and states > 0
    t.set_contains_nfa(1)
    assert t.contains_engine_name == table
    t.set_contains_nfa(2)
    assert t.contains_engine_name == "nfa-shift-and" and t.contains_states == states
    # the program is the lane program whatever engine the regex was compiled for
    ref = regex("ab+c").program(rr.PROGRAM_CONTAINS_NFA)
    for engine in (rr.ENGINE_NFA, rr.ENGINE_DFA):
        assert np.array_equal(rr.RRegex("ab+c", engine).program(rr.PROGRAM_CONTAINS_NFA), ref)


@pytest.mark.parametrize("pattern", [NEEDS_BOTH_REASONS] + [c.pattern for c in T.TOO_LARGE], ids=lambda p: p[:24])
def test_too_large_patterns_stay_unsupported(pattern):
    """Beyond 512 positions there is no lane program.  (a|b)*a(a|b){600} has no table either: unsupported at 1 and at 2, both reasons
    in the text.  a{1,600}b and the four x(p)y of 514 positions HAVE a contains table: option 1 keeps them on it, option 2 - the NFA
    always - has nothing to run, and says that the table is there but set aside, and that there is no lane program."""
    r = rr.RRegex(pattern)
    assert r.program(rr.PROGRAM_CONTAINS_NFA) is None
    has_table = r.contains_states > 0
    assert has_table == (pattern != NEEDS_BOTH_REASONS)
    for mode in (1, 2):
        r.set_contains_nfa(mode)
        if mode == 1 and has_table:
            assert r.contains_engine_name.startswith("dfa-")
            continue
        with pytest.raises(rr.RRegexError) as e:
            r.contains_engine_name
        text = str(e.value)
        assert "lane program" in text and "512 positions" in text
        assert ("set aside" in text) if has_table else ("determinise" in text)


def test_a_1_600_b_at_option_2():
    r = rr.RRegex("a{1,600}b")
    r.set_contains_nfa(2)
    with pytest.raises(rr.RRegexError, match="lane program"):
        r.contains_engine_name


# ---- the dump
def plain_replay(pattern):
    """the pattern's own lane program (RRX_ENGINE_NFA), where it was compiled"""
    w = rr.RRegex(pattern, rr.ENGINE_NFA).program(rr.ENGINE_NFA)
    return NfaReplay(w)


@pytest.mark.parametrize("pattern", [c.pattern for c in T.CASES] + T.TABLELESS + ["a\nb", "a*", "[]"], ids=lambda p: repr(p)[:28])
def test_the_dump_has_the_contains_rows(pattern):
    rep = replay(pattern)
    if pattern == "[]":                                    # the empty language: one dead position, nothing final
        assert rep.fin == 0 and all(b == 1 for b in rep.B)
        return
    own = plain_replay(pattern)
    assert (rep.W, rep.nbits, rep.n_exc) == (own.W, own.nbits, own.n_exc) and rep.init == 1
    for name in ("fin", "chain", "self_", "excm", "cgrp", "ctgt", "X"):
        assert getattr(rep, name) == getattr(own, name), name
    for c in range(256):
        assert rep.B[c] & 1, c                             # position 0 in every row ...
        if c == 0 or c >= 0x80:
            assert rep.B[c] == 1, c                        # ... alone in the rows of NUL and of the high bytes
        else:
            assert rep.B[c] == own.B[c] | 1 and not own.B[c] & 1, c       # (the '\n' row too: the pattern's own plus position 0)
    if pattern == "a\nb":
        assert rep.B[10] != 1


# ---- the replay against the expectations
@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id)
def test_replay_equals_the_expectation(case):
    rep = replay(case.pattern)
    lines, want = T.build(case)
    for final_newline in (True, False):
        got = rep.contains_lines(T.corpus(case, final_newline))
        assert got.shape == want.shape and np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    got = rep.contains_items(lines)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]


@pytest.mark.parametrize("pattern", T.TABLELESS)
def test_replay_equals_the_oracle_on_the_tableless_patterns(pattern):
    rep = replay(pattern)
    lines, want = T.tableless_lines(pattern), T.tableless_expected(pattern)
    assert 0 < int(want.sum()) < len(lines)
    assert np.array_equal(rep.contains_lines(b"\n".join(lines) + b"\n"), want)
    assert np.array_equal(rep.contains_items(lines), want)
    assert regex(pattern).contains_states == 0             # no table: what option 1 is for


def test_tableless_14_against_brute_force_on_short_lines():
    """lines of at most 22 bytes with NUL and high bytes among them: the oracle's brute-force search"""
    p = T.TABLELESS[0]
    rng = random.Random(14)
    lines = []
    for _ in range(300):
        t = bytearray("".join(rng.choice("aab") for _ in range(rng.choice((0, 3, 14, 15, 16, 20, 22)))).encode())
        if t and rng.random() < 0.3:
            t[rng.randrange(len(t))] = rng.choice((0, 0x80, 0xff, ord("-")))
        lines.append(bytes(t))
    lines.append(b"b")
    data = b"\n".join(lines) + b"\n"
    want = CC.brute_force(p, np.frombuffer(data, dtype=np.uint8))
    assert 0 < int(want.sum()) < len(lines)
    rep = replay(p)
    assert np.array_equal(rep.contains_lines(data), want) and np.array_equal(rep.contains_items(lines), want)


# ---- cross-checks of the composed expectation itself
SAMPLE = [c for k, c in enumerate(T.CASES) if k % 9 == 0]


@pytest.mark.parametrize("case", [c for c in SAMPLE if c.base.family != "carry"], ids=lambda c: c.id)
def test_expectation_equals_python_re(case):
    """((a?){n}b is left out: a backtracking matcher takes 2^n steps to reject a run of a's)"""
    lines, want = T.build(case)
    pat = re.compile(case.pattern.encode())
    got = np.array([1 if pat.search(t) else 0 for t in lines], dtype=np.uint8)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]


@pytest.mark.parametrize("case", [c for c in SAMPLE if c.base.family not in WC.SLOW_ORACLE or c.base.W <= 2][:5], ids=lambda c: c.id)
def test_expectation_equals_the_oracle(case):
    """the oracle's own automaton of .*(p).* on the ASCII lines, its brute-force search on the lines of at most 22 bytes"""
    lines, want = T.build(case)
    ascii_ = [i for i, t in enumerate(lines) if all(0 < c < 0x80 for c in t)][:60]
    assert np.array_equal(CC.dot_star(case.pattern, [lines[i] for i in ascii_]), want[ascii_])
    short = [i for i, t in enumerate(lines) if len(t) <= 22]
    if short:
        data = b"\n".join(lines[i] for i in short) + b"\n"
        if lines[short[-1]] == b"":
            data += b"\n"
        got = CC.brute_force(case.pattern, np.frombuffer(data, dtype=np.uint8))[:len(short)]
        assert np.array_equal(got, want[short])


# ---- reach and sharpness
def test_the_cases_reach_every_kernel():
    """ContainsLineNfaEngine<W, RULES> is chosen by the padded width and by n_exc (16 builds), contains_extents_nfa_kernel<W> by the
    padded width (8)"""
    line, items = set(), set()
    for case in T.CASES:
        rep = replay(case.pattern)
        line.add((WC.kernel_width(rep.W), rep.n_exc > 0))
        items.add(WC.kernel_width(rep.W))
    assert line == {(w, rules) for w in WC.KERNEL_WIDTHS for rules in (False, True)}
    assert items == set(WC.KERNEL_WIDTHS)
    assert {replay(p).W for p in T.TABLELESS} == {1, 2, 5}


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id)
def test_the_lines_are_sharp(case):
    rep = replay(case.pattern)
    lines, want = T.build(case)
    data = T.corpus(case)
    for drop in ("a", "b", "c", "top"):
        assert not np.array_equal(rep.contains_lines(data, drop), want), drop
    for drop in ("a", "c", "top"):
        assert not np.array_equal(rep.contains_items(lines, drop), want), drop
