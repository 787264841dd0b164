"""The group, wave and sparse NFA engines' instantiation matrix on the CPU (case table: coop_engine_cases.py): every case lowers to a
program from which pack.cpp's rules and the dispatchers of kernels_coop.hip / kernels_wave.hip choose the instantiation the table
names, the cases together reach every instantiation the front end can reach, the closed forms are the oracle's language at a small
size, NfaReplay and the layout replay (program_replay.CoopReplay) of every dump give the closed form's verdicts, and every mutant of
the layout replay - one wrong step of a kernel at a time - changes a verdict of every case whose build it applies to.  The GPU test
(test_coop_engines_gpu.py) runs the kernels on the same lines, so a change of the lowering that moves a case to another kernel fails
HERE.  No GPU needed."""
import os

import numpy as np
import pytest

import coop_engine_cases as T
import roaringregex_amd as rr
from program_replay import CoopReplay, NfaReplay
from pyoracle import OracleRegex

_programs = {}


def popcount(v):
    return bin(v).count("1")


def word_bits(mask, W, per):
    """bit i: some word w of the set with w % per == i is not zero in `mask`"""
    out = 0
    for w in range(W):
        if (mask >> (32 * w)) & 0xffffffff:
            out |= 1 << (w % per)
    return out


def program(case):
    """-> (NfaReplay of the CSR dump, number of byte classes, words_per_set)"""
    if case.id not in _programs:
        assert (rr.ENGINE_NFA_WAVE, rr.ENGINE_NFA_BLOCK, rr.ENGINE_NFA_SPARSE) == (T.ENGINE_NFA_WAVE, T.ENGINE_NFA_BLOCK, T.ENGINE_NFA_SPARSE)
        e = T.ENGINE_OF[case.engine]
        r = rr.RRegex(case.pattern, e)
        assert r.engine == e and r.engine_name == T.ENGINE_NAME[case.engine], (case.id, r.engine_name)
        if case.engine == "group":
            # the group engine's dump carries dense exception rows (up to 4096 positions): masks and B rows are the CSR dump's, the rows
            # are the lists
            dense = r.program(e)
            csr = rr.RRegex(case.pattern, rr.ENGINE_NFA_BLOCK).program(rr.ENGINE_NFA_BLOCK)
            head = 4 + 263 * int(dense[0])
            assert (dense[:head] == csr[:head]).all(), case.id
            rep = NfaReplay(csr, sparse=True)
            if rep.n_exc and case.nbits <= 1100:            # (the small ones: a dense dump of 4096 positions is two million words)
                assert NfaReplay(dense).X == rep.X, case.id
        else:
            rep = NfaReplay(r.program(e), sparse=True)
        assert r.words_per_set == rep.W
        _programs[case.id] = (rep, r.byte_classes, r.words_per_set)
    return _programs[case.id]


def class_rows(rep, ncls):
    """the B rows of the byte classes 1 ... ncls - 1 (a class is the bytes with one row; class 0: no row)"""
    rows = {rep.B[c] for c in range(1, 128)} - {0}
    assert len(rows) == ncls - 1 and ncls <= T.MAX_CLASSES and not any(rep.B[c] for c in [0] + list(range(128, 256)))
    return rows


def derive(case):
    """pack.cpp (pack_group_nfa, pack_wave_nfa), device.hpp (group_geometry), kernels_wave.hip (wave_words_per_lane, sparse_rows) and the
    six dispatchers, recomputed from the dump -> (instantiation, the fields it was chosen by)"""
    rep, ncls, _ = program(case)
    W, N = rep.W, rep.nbits
    assert rep.cgrp == 0 and rep.ctgt == 0 and rep.init == 1 and popcount(rep.excm) == rep.n_exc
    if case.engine == "group":
        G, K = T.group_geometry(N)
        self_slots, exc_slots, b_slots = word_bits(rep.self_, W, K), word_bits(rep.excm, W, K), 0
        rows = class_rows(rep, ncls)
        for w in range(G * K):
            used = 0 if w * 32 >= N else 0xffffffff if N - w * 32 >= 32 else (1 << (N - w * 32)) - 1
            if any(((row >> (32 * w)) & used) != used for row in rows):
                b_slots |= 1 << (w % K)
        exc_mode = 2 if rep.excm == 1 else 0                # one exception row, and it is position 0's
        slot0 = ((b_slots | self_slots) & ~1) == 0
        inst = ("group", G, K, exc_mode, slot0 if exc_mode == 2 else False)
        return inst, dict(G=G, K=K, exc_mode=exc_mode, self_slots=self_slots, b_slots=b_slots, exc_slots=exc_slots, slot0=slot0)
    if case.engine == "wave":
        WL = T.wave_words_per_lane(W)
        self_words, exc_words = word_bits(rep.self_, W, WL), word_bits(rep.excm, W, WL)
        front = not (self_words & ~1) and not (exc_words & ~1)
        return ("wave", WL, front), dict(WL=WL, self_words=self_words, exc_words=exc_words, front=front)
    WR = T.sparse_rows(W)
    class_rows(rep, ncls)
    lrows = ncls * WR * 64 * 4 <= T.SPARSE_LDS_BUDGET
    return ("sparse", WR, lrows), dict(WR=WR, ncls=ncls, lrows=lrows, self_words=word_bits(rep.self_, W, WR), exc_words=word_bits(rep.excm, W, WR))


def layout(case, mutant=None):
    rep = program(case)[0]
    inst, f = derive(case)
    if case.engine == "group":
        return CoopReplay(rep, "group", f["G"], f["K"], slot0=inst[4], mutant=mutant)
    return CoopReplay(rep, case.engine, 64, inst[1], mutant=mutant)


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id)
def test_case_reaches_the_instantiation_the_table_names(case):
    rep = program(case)[0]
    inst, f = derive(case)
    assert rep.nbits == case.nbits == T.positions(case.family, case.n), (case.pattern, rep.nbits)
    assert inst == case.inst, (case.pattern, inst, f)
    beyond = ~((1 << rep.nbits) - 1)
    for name in ("init", "fin", "self_", "excm"):
        assert getattr(rep, name) & beyond == 0, name
    assert all(b & beyond == 0 for b in rep.B) and all(x & beyond == 0 for x in rep.X)
    assert not any(b & 1 for b in rep.B), "position 0 is in no B row: a 1 that arrives there mid-line survives no byte"
    if case.engine == "group":
        G, K = f["G"], f["K"]
        if case.edge == "full":
            assert 32 * G * K - rep.nbits <= 2 and (rep.fin >> (rep.nbits - 1)) & 1, "the last slot's top bits in use, the top position final"
        if case.edge == "low":
            prev = max([32 * g * k for g, k in T.GROUP_FORMS if 32 * g * k < 32 * G * K] + [T.GROUP_MIN_BITS - 1])
            assert prev < rep.nbits <= prev + 4
        # the branches inside one build: <0, false> without self loops and exceptions, with a self loop in the top slot and exc_slots ==
        # 0, with exceptions in every slot; <2, false> with masks in every slot
        if case.family == "chain1":
            assert (f["self_slots"], f["exc_slots"], rep.n_exc) == (0, 0, 0)
        if case.family == "selfhi":
            assert f["exc_slots"] == 0 and popcount(rep.self_) == 1 and (case.edge != "full" or f["self_slots"] == 1 << (K - 1))
        if case.family in ("exc", "star"):
            assert f["exc_slots"] == (1 << K) - 1 if case.family == "exc" else f["exc_slots"] & ~1
        if case.family == "bstar":
            assert f["b_slots"] == (1 << K) - 1 and f["self_slots"] == 1 and f["exc_slots"] == 1
    elif case.engine == "wave":
        WL = f["WL"]
        if case.edge == "full":
            assert rep.W == 64 * WL and rep.nbits == 2048 * WL
        if case.edge == "low":
            assert rep.W == 64 * max(w for w in T.WAVE_WIDTHS if w < WL) + 1
        if case.family == "selfhi":
            assert f["self_words"] & ~1 and not f["exc_words"], "!FRONT by the self term alone"
        if case.family == "exc":
            assert f["exc_words"] & ~1 and not f["self_words"], "!FRONT by exception positions alone"
        if case.family in ("chain1", "chainx"):
            assert not f["exc_words"] and not f["self_words"], "any_exc == 0"
        if case.family in ("carry3", "bstar", "heads"):
            assert f["exc_words"] == 1, "FRONT with the exception scan"
    else:
        if case.family in ("exc",):
            assert f["WR"] >= 2 and max(len(bin(x)) - 2 for x in rep.X) // 2048 >= 1, "edges into other blocks"
    ls = T.lines(case)
    # what the stripes kernels need of the corpus: a '\n' on every byte of a 16-byte chunk in turn, a dead line longer than a stripe of
    # 1024, empty lines, a last line that is not empty; the full group cases begin with the two lines of neighbouring groups
    data = T.corpus(case)
    nl = [i for i, c in enumerate(data) if c == 10]
    gaps = [q - p for p, q in zip(nl, nl[1:])]
    assert any(all(g == 17 for g in gaps[i:i + 15]) for i in range(len(gaps) - 14))
    outside = {t[0] for t in ls if len(t) > 1024 and not rep.B[t[0]]}
    assert outside and b"" in ls and ls[-1]
    if case.engine == "group" and case.edge == "full" and case.family != "star":
        assert T.accepts(case, ls[0]) and len(ls[0]) == max(len(t) for t in ls if T.accepts(case, t))   # (the top position is final)
        second = ls[2] if len(ls[0]) < 1023 else ls[1]
        assert data.index(second) == max(1024, len(ls[0]) + 1) and not T.accepts(case, second) and T.accepts(case, second[1:])
    assert len(ls) <= 130 and max(len(t) for t in ls) <= case.nbits + 1200 and sum(len(t) + 1 for t in ls) <= 40 * (case.nbits + 1200)


def test_cases_reach_every_reachable_instantiation():
    """24 group forms, 19 wave-resident forms (WaveNfa<1, false> is never chosen: one word per lane is word 0) less WL 32, 12 sparse forms
    less <1, false>: each with a stripes and an extents kernel.  What is left out is left out because the front end cannot get there:
    test_the_front_end_refuses_what_would_select_wl32."""
    got = {derive(case)[0] for case in T.CASES}
    assert got == T.REACHABLE, (sorted(T.REACHABLE - got), sorted(got - T.REACHABLE))
    assert len([i for i in T.REACHABLE if i[0] == "group"]) == 24 and len([i for i in T.REACHABLE if i[0] == "wave"]) == 17
    assert len([i for i in T.REACHABLE if i[0] == "sparse"]) == 11
    # every group form at both ends of its range in every build
    ends = {(c.inst, c.edge) for c in T.CASES if c.engine == "group"}
    assert {(("group", G, K, m, s), e) for G, K in T.GROUP_FORMS for m, s in T.GROUP_BUILDS for e in ("full", "low")} <= ends
    for G, K in T.GROUP_FORMS:
        fams = {c.family for c in T.CASES if c.inst[:3] == ("group", G, K)}
        assert {"carry3", "bstar", "chain1", "selfhi", "exc"} <= fams
    assert {c.inst[1] for c in T.CASES if c.family == "star"} == {16, 32}
    # the wave engine: both edges of the chain at every width, both ways out of FRONT at every width >= 2 their families reach
    for WL in T.WAVE_WIDTHS[:-1]:
        edges = {c.edge for c in T.CASES if c.inst == ("wave", WL, True) and c.family in ("chain1", "chainx")}
        assert edges == {"full", "low"} - ({"low"} if WL == 1 else set()) - ({"full"} if WL == 24 else set()), WL
        if WL >= 2:
            fams = {c.family for c in T.CASES if c.inst == ("wave", WL, False)}
            assert fams == {"selfhi", "exc"} - ({"exc"} if WL == 24 else set()), WL
        assert any(c.inst == ("wave", WL, True) and c.family in ("carry3", "bstar", "heads") for c in T.CASES) or WL == 24
    assert any(c.engine == "sparse" and c.family == "exc" and c.inst[1] >= 2 for c in T.CASES)


def test_the_front_end_refuses_what_would_select_wl32():
    """WaveNfa<32, .> holds 49 153 ... 65 536 positions.  The front end refuses more than 65 536 reference states and the reference spends
    at least two states on a position, so no pattern gets there: the smallest member of every family that would is refused, and the
    largest chain that is admitted - a{32768}, 32 769 positions - runs at 24 words per lane.  That size is where the sparse form's 32
    rows BEGIN (it has no 24): SparseNfa<32, .> is reached, and has cases.  SparseNfa<1, false> would need more byte classes than
    there are."""
    assert T.wave_words_per_lane((49153 + 31) // 32) == 32 and T.wave_words_per_lane((49152 + 31) // 32) == 24
    for p in T.BEYOND_THE_FRONT_END:
        for e in (rr.ENGINE_NFA_BLOCK, rr.ENGINE_NFA_SPARSE):
            with pytest.raises(rr.RRegexError, match="too many states"):
                rr.RRegex(p, e)
    r = rr.RRegex("a{32768}", rr.ENGINE_NFA_BLOCK)
    assert r.states_n == 65536 and r.words_per_set == 1025 and T.wave_words_per_lane(1025) == 24 and T.sparse_rows(1025) == 32
    for p in ("a{32769}", "a{32768}b", "b?a{32768}", ".{32769}"):
        with pytest.raises(rr.RRegexError, match="too many states"):
            rr.RRegex(p, rr.ENGINE_NFA_BLOCK)
    assert T.MAX_CLASSES * 1 * 64 * 4 <= T.SPARSE_LDS_BUDGET


@pytest.mark.parametrize("family", sorted(T.SMALL), ids=str)
def test_closed_form_is_the_oracles_language(family):
    """The closed form of a family against OracleRegex at a small member of the family, on the lines the table would run there (and on
    every line of two letters up to a length)."""
    n = T.SMALL[family]
    o = OracleRegex(T.pattern_of(family, n))
    import random
    rng = random.Random(family)
    ls = T._family_lines(family, n, ("group", 8, 3, 0, False), rng) + [T._short(family, n, rng), b"", b"a", b"b", b"ab", b"ba", b"aab", b"abab", b"abba"]
    for L in range(0, 10):
        ls += [bytes(rng.choice(b"ab") for _ in range(L)) for _ in range(8)]
    if family == "heads":
        H = T._heads(n[0])
        ls += [H[i:i + 3] + b"a" * n[1] for i in range(len(H))] + [H[i:i + 1] + H[i - 1:i] + b"a" * n[1] for i in range(1, len(H))]
    got = [T.accepts(family, t, n) for t in ls]
    want = [o.accepts(t) for t in ls]
    assert got == want, [t for t, g, w in zip(ls, got, want) if g != w][:3]
    assert 1 <= sum(want) <= len(want) - 3                   # (a{n} has one member)


def verdicts(replay, ls):
    return np.array([1 if replay.accepts(t) else 0 for t in ls], dtype=np.uint8)


def first_bad(case, got, want, ls, what):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (case.pattern, case.inst, what, "first bad line", int(bad[0]), len(ls[bad[0]]), ls[bad[0]][-40:], "got", int(got[bad[0]]))


# the engines whose step has the step a mutant gets wrong
MUTANT_ENGINES = {"a": ("group", "wave", "sparse"), "b": ("group", "wave", "sparse"), "c": ("group",), "d": ("sparse",), "e": ("group",), "f": ("group",),
                  "g": ("group", "wave", "sparse")}


def applies(case, m, f, rep):
    """Does mutant m change the step of this case's build?  Where it does not, the program (or the geometry) makes it a no-op, and
    the test asserts THAT instead."""
    if m == "a":
        return rep.self_ >> 2048 != 0 if case.engine == "sparse" else bool(f.get("self_slots", f.get("self_words", 0)) & ~1)
    if m == "b":
        return rep.excm >> 2048 != 0 if case.engine == "sparse" else bool(f.get("exc_slots", f.get("exc_words", 0)) & ~1)
    # c, d: the position at the boundary must be one the shift enters at all (CHAIN: a path head is entered by exception edges only - in
    # (ab|ba){1,k} every position 4j + 4 is one, and so is every multiple of 2048)
    if m == "c":
        return f["G"] == 32 and bool((rep.chain >> (32 * f["K"] * 16)) & 1)
    if m == "d":
        return any((rep.chain >> p) & 1 for p in range(2048, rep.nbits, 2048))
    if m == "e":
        return any(b & 1 for b in rep.B)                     # (never: position 0 is in no B row, the 1 survives no byte)
    if m == "f":
        return True
    return rep.nbits % 32 != 0                               # g: the top word has bits beyond nbits


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id)
def test_replays_give_the_reference_and_every_mutant_is_caught(case):
    """NfaReplay of the dump - plain form line by line, match_lines over the corpus with and without its final newline - and the layout
    replay give the reference's verdicts (the closed form's; the oracle's for the two-branch star); then each mutant of the layout
    replay that applies to the case's build must change a verdict.  Neither all-0 nor all-1 would pass."""
    rep = program(case)[0]
    f = derive(case)[1]
    ls, want = T.lines(case), T.expected(case)
    assert len(want) == len(ls) and 1 <= int(want.sum()) <= len(ls) - 3
    edge = T.edge_lines(case)
    assert want[edge].any() and not want[edge].all()
    first_bad(case, verdicts(rep, ls), want, ls, "NfaReplay, plain form")
    first_bad(case, np.array(rep.match_lines(T.corpus(case)), dtype=np.uint8), want, ls, "NfaReplay.match_lines")
    assert rep.match_lines(T.corpus(case, False)) == list(want)
    base = layout(case)
    first_bad(case, verdicts(base, ls), want, ls, "layout replay")
    # (the lines a mutant is likely to get wrong first: those with a byte outside the classes, then the members, short before long)
    order = sorted(range(len(ls)), key=lambda i: (not (set(ls[i]) - set(b"ab") or want[i]), len(ls[i])))
    for m in CoopReplay.MUTANTS:
        if case.engine not in MUTANT_ENGINES[m]:
            continue                                         # (that engine's step has no such part)
        if applies(case, m, f, rep):
            mut = layout(case, m)
            assert any(mut.accepts(ls[i]) != bool(want[i]) for i in order), (case.id, case.inst, "mutant", m, "changes no verdict: the lines are not sharp")
        elif m == "c" and f["G"] < 32:
            pass                                             # a group of 8 or 16 lanes lies inside one DPP row
        else:
            # a no-op by the program: the same masks; the carries it drops go into positions the shift never enters; the 1 it lets
            # into position 0 survives no B row
            mut = layout(case, m)
            live = (1 << rep.nbits) - 1
            assert (mut.fin, mut.self_, mut.excm, mut.unmasked, mut.flag) == (base.fin, base.self_, base.excm, base.unmasked, base.flag), (case.id, m)
            assert (base.keep ^ mut.keep) & live & rep.chain == 0, (case.id, m)
            assert mut.B == base.B and not any(b & 1 for b in mut.B), (case.id, m)


def test_documents_name_files_of_this_matrix_that_exist():
    tests = os.path.dirname(os.path.abspath(__file__))
    text = open(os.path.join(tests, "..", "DESIGN.md")).read()
    for name in ("coop_engine_cases.py", "test_coop_engines_lowering.py", "test_coop_engines_gpu.py"):
        assert "`" + name + "`" in text, name
        assert os.path.exists(os.path.join(tests, name)), name
    for case in T.CASES:                                     # DESIGN's table names the cases that reach each instantiation
        assert "`" + case.id + "`" in text, case.id
