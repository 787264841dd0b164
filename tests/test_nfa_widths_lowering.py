"""The NFA lane engine's width-by-build matrix on the CPU (case table: nfa_width_cases.py): every case lowers to the program the table
says - width, flags, word-boundary properties -, the cases together reach every kernel build, and the replay of each program equals
the oracle on the case's lines.  The GPU test (test_nfa_widths_gpu.py) compares the kernels with the same vectors, so a change of the
lowering that moves a case to another kernel fails HERE.  No GPU needed.

That the table bites was checked with three defects put into program_replay.NfaReplay (both step functions), one at a time; the
cases of test_replay_equals_the_oracle that failed:
  * the carry dropped between the words of the multiword add: carry-W2-n52 ... carry-W16-n500 (all fifteen (a?){n}b of two words or
    more: one run across every word boundary), mix2-W4-n31 and mix2-W16-n127 (a run across the last boundary); the runs of b*a{1,n}
    and (a|b)*a(a|b){n} lie inside a word and do not notice
  * bit 31 of the top word masked out of FIN: chain-W1-n31, -W2-n63, -W4-n127, -W5-n159, -W7-n223, -W8-n255, -W11-n351, -W12-n383,
    -W15-n479, -W16-n511 (the ten chains of nbits == 32 W), self2-W2-n62, self2-W12-n382, self2-W16-n510 and carry2-W16-n510 (the other
    programs whose last position is bit 31 of the top word)
  * exception rows whose target word is not their source word cut to their source word: all thirty exc and mix cases of two words or
    more, and the four mix2 cases"""
import numpy as np
import pytest

import nfa_width_cases as T
import roaringregex_amd as rr
from program_replay import NfaReplay, SampledReplay
from pyoracle import OracleRegex

_replays = {}


def replay(case):
    if case.id not in _replays:
        r = rr.RRegex(case.pattern, rr.ENGINE_NFA)
        assert r.engine == rr.ENGINE_NFA and r.engine_name == "nfa-shift-and"
        _replays[case.id] = NfaReplay(r.program(rr.ENGINE_NFA))
        assert r.words_per_set == _replays[case.id].W
    return _replays[case.id]


def bit(v, i):
    return (v >> i) & 1


def cross_word_rows(rep):
    """exception positions with a target in another word than their own"""
    out = []
    e = rep.excm
    while e:
        b = (e & -e).bit_length() - 1
        e &= e - 1
        row, words = rep.X[b], set()
        for w in range(rep.W):
            if (row >> (32 * w)) & 0xffffffff:
                words.add(w)
        if words - {b >> 5}:
            out.append(b)
    return out


def straddled_boundaries(rep):
    """k with bits 32k - 1 and 32k both in CGRP: one run of the multiword add, its carry crosses from word k - 1 into word k"""
    return [k for k in range(1, rep.W) if bit(rep.cgrp, 32 * k - 1) and bit(rep.cgrp, 32 * k)]


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id)
def test_case_lowers_to_the_program_the_table_names(case):
    rep = replay(case)
    assert (rep.W, rep.nbits) == (case.W, case.nbits), (case.pattern, rep.W, rep.nbits)
    assert rep.init == 1 and not rep.accepts_empty
    flags = (rep.n_exc > 0, rep.cgrp != 0, rep.self_ != 0)
    assert (rep.n_exc > 0) == (rep.excm != 0) and (rep.cgrp != 0) == (rep.ctgt != 0)
    if case.shape == "chain":
        assert flags == (False, False, False)
    elif case.shape == "self":
        assert flags == (False, False, True)
    elif case.shape == "carry":
        assert flags[:2] == (False, True)
    elif case.shape == "exc":
        assert flags[:2] == (True, False)
    else:
        assert case.shape == "mix" and flags[:2] == (True, True)
    # the padded widths rely on it: nothing of the program lies beyond its own positions
    beyond = ~((1 << rep.nbits) - 1)
    for name in ("init", "fin", "chain", "self_", "excm", "cgrp", "ctgt"):
        assert getattr(rep, name) & beyond == 0, name
    assert all(b & beyond == 0 for b in rep.B) and all(x & beyond == 0 for x in rep.X)
    if case.family == "chain" and case.nbits == 32 * case.W:
        assert bit(rep.fin, 32 * case.W - 1), "the top word's bit 31 is in use and final"
    if case.family == "chain" and case.nbits == 32 * (case.W - 1) + 1:
        assert bit(rep.fin, 32 * (case.W - 1)) and rep.fin >> (32 * (case.W - 1)) == 1, "only bit 0 of the top word, and final"
    if case.family == "carry" and case.W >= 2:
        assert straddled_boundaries(rep) == list(range(1, case.W)), "(a?){n}b: one run across every word boundary"
    if case.shape in ("exc", "mix") and case.W >= 2:
        assert cross_word_rows(rep), "an exception row with a target in another word"
    assert len(T.corpus(case)) <= T.MAX_CORPUS_BYTES
    assert len(T.lines(case)) > T.RANDOM_LINES + 100


def test_cases_reach_every_width_and_every_build():
    """All 32 batch kernels and all 24 one-pass kernels (kernel width x build), every program width 1 ... 16 in every shape, the chain
    cut to nbits == 32 W and to 32 (W - 1) + 1 at the EDGE_WIDTHS, a carry group across a word boundary at several of them, the
    exception build with the carry flag off and on at every width."""
    batch, onepass, shapes, widths = set(), set(), set(), set()
    full, bit0, straddled, exc_flag = set(), set(), set(), set()
    for case in T.CASES:
        rep = replay(case)
        kw = T.kernel_width(rep.W)
        batch.add((kw, T.batch_build(rep.n_exc, rep.cgrp, rep.self_)))
        onepass.add((kw, T.onepass_build(rep.n_exc, rep.cgrp, rep.self_)))
        shapes.add((case.shape, rep.W))
        widths.add(rep.W)
        if case.family == "chain" and rep.nbits == 32 * rep.W and bit(rep.fin, rep.nbits - 1):
            full.add(rep.W)
        if case.family == "chain" and rep.nbits == 32 * (rep.W - 1) + 1:
            bit0.add(rep.W)
        straddled.update(straddled_boundaries(rep))
        if rep.n_exc:
            exc_flag.add((rep.W, rep.cgrp != 0))
    assert batch == {(w, b) for w in T.KERNEL_WIDTHS for b in T.BATCH_BUILDS} and len(batch) == 32
    assert onepass == {(w, b) for w in T.KERNEL_WIDTHS for b in T.ONEPASS_BUILDS} and len(onepass) == 24
    assert widths == set(range(1, 17))
    assert shapes == {(s, w) for s in ("chain", "self", "carry", "exc", "mix") for w in range(1, 17)}
    assert full == set(T.EDGE_WIDTHS) and bit0 == set(T.EDGE_WIDTHS[1:])
    assert straddled == set(range(1, 16))
    assert exc_flag == {(w, f) for w in range(1, 17) for f in (False, True)}
    # self loops WITHOUT carry groups at sixteen words: the build test_nfa_lane_engine_sixteen_words' patterns do not reach
    assert any(T.kernel_width(c.W) == 16 and c.shape == "self" for c in T.CASES)
    assert len({c.id for c in T.CASES}) == len(T.CASES)


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id)
def test_replay_equals_the_oracle(case):
    """NfaReplay.match_lines (line mode: what LineNfaEngine steps) over the whole corpus, with and without a final newline, and
    NfaReplay.accepts (plain mode: NfaCore::advance, what the extents and recheck kernels step) line by line, against the oracle;
    neither all-0 nor all-1 would pass."""
    rep = replay(case)
    lines, want = T.lines(case), T.expected(case)
    assert len(want) == len(lines) and 0 < int(want.sum()) < len(lines), (case.id, int(want.sum()))
    assert not want[[i for i, t in enumerate(lines) if b"\x00" in t or b"\xc3" in t]].any()
    assert want[T.edge_lines(case)].any() and not want[T.edge_lines(case)].all()
    for final_newline in (True, False):
        got = np.array(rep.match_lines(T.corpus(case, final_newline)), dtype=np.uint8)
        assert got.shape == want.shape
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (case.pattern, "line mode", "first bad line", int(bad[0]), len(lines[bad[0]]), lines[bad[0]][-50:])
    got = np.array([1 if rep.accepts(t) else 0 for t in lines], dtype=np.uint8)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (case.pattern, "plain mode", "first bad line", int(bad[0]), len(lines[bad[0]]), lines[bad[0]][-50:])


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id)
def test_recorded_vectors_are_the_oracles(case):
    """tests/golden/nfa_width_vectors.json against the live oracle: every line, but for the wide programs of the families whose
    reference automaton has n * n / 2 edges (nfa_width_cases.SLOW_ORACLE) - there every seventh line and lines of the edge lengths."""
    idx = T.oracle_sample(case)
    want = T.expected(case)
    got = T.oracle_vector(case, idx)
    assert (got == (want if idx is None else want[idx])).all(), case.id


@pytest.mark.parametrize("n,W", T.SAMPLED_CASES, ids=lambda v: str(v))
def test_sampled_table_is_learnt_at_this_width(n, W):
    """[a-c]{1,6}:(x|y)*x(x|y){n}: AUTO leaves it on the NFA lane engine at the width the table names, learn_table installs a table from
    the short sample, and of the corpora the GPU test runs exactly the lines built to escape end in the ESCAPE state - few enough for the
    list in one, too many for it in the other, never enough to retire the table; the lines the table decides have the oracle's verdict."""
    pattern = T.sampled_pattern(n)
    r = rr.RRegex(pattern)
    assert r.engine == rr.ENGINE_NFA and r.engine_name == "nfa-shift-and" and r.words_per_set == W and r.sampled_table is None
    assert T.kernel_width(W) in (6, 12, 16)
    states, open_tr = r.learn_table(T.sampled_sample())
    assert 10 < states < 200 and open_tr > 0
    rep = SampledReplay(r.program(rr.PROGRAM_SAMPLED_DFA), r.program(rr.PROGRAM_SAMPLED_DFA2))
    o = OracleRegex(pattern)
    corpora = [("list", stripe, T.sampled_few(n, stripe)[:2]) for stripe in (1024, 4096)] + [("walk", 0, T.sampled_many(n))]
    for name, stripe, (data, escaping) in corpora:
        ls = data.split(b"\n")[:-1]
        verdicts = [rep.verdict(t) for t in ls]
        assert [i for i, v in enumerate(verdicts) if v is None] == escaping, name
        assert all(v == int(o.accepts(t)) for v, t in zip(verdicts, ls) if v is not None), name
        cap = T.sampled_list_capacity(len(ls))
        assert cap == T.SAMPLED_LIST_FLOOR and (len(escaping) <= cap) == (name == "list")
        assert len(escaping) * 100 <= len(ls) * T.SAMPLED_RETIRE_PERCENT
        if name == "list":
            assert 0 in escaping and len(ls) - 1 in escaping and max(len(ls[i]) for i in escaping) > stripe
    assert {T.kernel_width(w) == w for _, w in T.SAMPLED_CASES} == {True, False}, "an exact and a padded width"


def test_design_names_files_of_this_matrix_that_exist():
    """DESIGN.md's paragraph on which test launches which kernel names these files without their directory."""
    import os
    tests = os.path.dirname(os.path.abspath(__file__))
    text = open(os.path.join(tests, "..", "DESIGN.md")).read()
    for name, where in (("nfa_width_cases.py", ""), ("test_nfa_widths_lowering.py", ""), ("test_nfa_widths_gpu.py", ""),
                        ("nfa_width_vectors.json", "golden"), ("make_nfa_width_vectors.py", "golden")):
        assert "`" + name + "`" in text, name
        assert os.path.exists(os.path.join(tests, where, name)), name
