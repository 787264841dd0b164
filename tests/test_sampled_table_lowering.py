"""The sampled-table cases on the CPU (case table: sampled_table_cases.py): the pattern and its table are what the table says, every
case's escaping lines are exactly the lines the table does not decide, the replay of the two-bit stride-2 form equals the oracle on
every case of at most 1 MiB, no case hides behind the retire rule or leaves the sampled path, and every case HAS the property it is
named for - the dense slot, the tail of '\\n' pairs, the straddling line and its pair, the shared wide word, the words beyond the
window, the split's block and turn, the escaped total on either side of the cap, the place of the '\\n' in front of a listed line, the
stripe without a line start.  The GPU test (test_sampled_table_gpu.py) runs the kernels on the same bytes, so a change that moves a
case off its edge fails HERE.  No GPU needed."""
import numpy as np
import pytest

import roaringregex_amd as rr
import sampled_table_cases as T
from program_replay import SampledReplay
from pyoracle import OracleRegex

_state = {}


def table():
    """(the replay of the learnt table, the oracle) - learnt once"""
    if not _state:
        r = rr.RRegex(T.PATTERN)
        assert r.engine == rr.ENGINE_NFA and r.engine_name == "nfa-shift-and" and r.words_per_set == 2 and r.accepts_empty
        assert r.sampled_table is None
        states, open_tr = r.learn_table(T.sample())
        assert 10 < states < 60 and open_tr > 0
        _state["rep"] = SampledReplay(r.program(rr.PROGRAM_SAMPLED_DFA), r.program(rr.PROGRAM_SAMPLED_DFA2))
        _state["oracle"] = OracleRegex(T.PATTERN)
    return _state["rep"], _state["oracle"]


def lines_of(b):
    raw = b.data.tobytes().split(b"\n")
    return raw[:-1] if b.final_newline else raw


def test_pattern_and_table_have_the_four_properties():
    """Nullable, on the NFA lane engine under AUTO, a table that decides lines of 0 and 1 bytes with both verdicts, and an escaping
    line of at most 16 bytes; the escaping lines are accepted exactly when an x stands 41 bytes from their end."""
    rep, o = table()
    for t in T.DECIDED:
        assert rep.verdict(t) == (1 if o.accepts(t) else 0), t
    assert [rep.verdict(t) for t in T.DECIDED] == [1, 1, 1, 1, 0, 0, 0, 0, 0]
    assert rep.verdict(b"") == 1 and rep.verdict(b"a") == 1 and rep.verdict(b"d") == 0
    assert rep.verdict(b"x" * 11) == 0 and rep.verdict(T.ER) is None and len(T.ER) <= 16 and not o.accepts(T.ER)
    assert rep.verdict(T.EA) is None and o.accepts(T.EA)
    for length in (53, 60, 61, 187, 1084, 8252):
        for accept in (True, False):
            t = T.esc(length, accept)
            assert rep.verdict(t) is None and o.accepts(t) == accept, (length, accept)
    # a NUL leads to the table's dead state from every state, ESCAPE included: neither line escapes, the table rejects both
    assert rep.verdict(T.NUL_INSIDE) == 0 and not o.accepts(T.NUL_INSIDE) and rep.verdict(T.NUL_INSIDE[:20]) is None
    assert rep.verdict(T.NUL_IN_FRONT) == 0 and not o.accepts(T.NUL_IN_FRONT)
    assert rep.verdict(T.ER_CLASS1) is None and not o.accepts(T.ER_CLASS1)


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id)
def test_case_is_pinned_to_the_references(case):
    rep, o = table()
    b = T.built(case)
    nlines = len(b.idx)
    assert int(b.data.max()) < 0x80, "a byte >= 0x80 leaves the sampled path"
    assert int((b.data == 10).sum()) + (0 if b.final_newline else 1) == nlines
    verdict = [rep.verdict(v) for v in b.vocab]
    escapes = np.array([v is None for v in verdict])[b.idx]
    assert np.array_equal(np.nonzero(escapes)[0], b.escaping), "the escaping lines are exactly the ones built to escape"
    want = T.expected(case, o)
    for k, v in enumerate(verdict):
        assert v is None or v == (1 if o.accepts(b.vocab[k]) else 0), (case.id, b.vocab[k][:20])
    esc_want, dec_want = want[b.escaping], np.delete(want, b.escaping)
    if case.both_verdicts:
        assert esc_want.any() and not esc_want.all(), "both verdicts among the escaping lines"
    if nlines > 1:
        assert dec_want.any() and not dec_want.all(), "both verdicts among the lines the table decides"
    assert len(b.escaping) * 100 <= nlines * T.RETIRE_PERCENT, "the case would retire the table"
    cap = T.list_capacity(nlines)
    assert (len(b.escaping) <= cap) == (case.path == "list"), (len(b.escaping), cap)
    assert all(s == 0 or (T.MIN_STRIPE <= s <= T.MAX_STRIPE and s & (s - 1) == 0) for s in case.stripes)
    if len(b.data) <= T.REPLAY_LIMIT:
        ls = lines_of(b)
        assert len(ls) == nlines and all(ls[i] == b.vocab[b.idx[i]] for i in range(0, nlines, max(nlines // 500, 1)))
        assert np.array_equal(o.match_lines(b.data), want), "the oracle over the whole text"
        per_line = [verdict[k] for k in b.idx]
        assert rep.match_lines2(b.data.tobytes()) == per_line, "the replay of the two-bit form"
    else:
        assert case.group == "B3", "one large case"


def newline_offsets(b):
    return np.nonzero(b.data == 10)[0]


def test_a1_has_sixteen_line_ends_in_a_slot_at_every_residue():
    (case,) = T.of_group("A1")
    b = T.built(case)
    assert len(b.data) % 4096 == 0, "whole rounds at every stripe"
    is_nl = (b.data == 10)
    per8 = is_nl.reshape(-1, 8).sum(axis=1)
    per16 = is_nl.reshape(-1, 16).sum(axis=1)
    assert (per8 == 8).any() and (per16 == 16).any()
    residues = {kind: set() for kind in range(4)}
    for off, kind in b.notes["runs"]:
        assert b.data[off - 1] == 10
        residues[kind].add(off % 16)
        if kind == 0:
            assert is_nl[off:off + 64].all() and b.data[off - 2] != 10
        elif kind in (1, 2):
            assert bytes(b.data[off:off + 80]) == (b"a\n" if kind == 1 else b"d\n") * 40
    assert all(residues[kind] == set(range(16)) for kind in range(4))
    # a slot of sixteen line ends follows a slot that left results in the register, and one that left none, in some stripe's lane
    full = np.nonzero(per16 == 16)[0]
    assert len(full) >= 16 * 3


def test_a2_tails_are_newline_pairs_of_both_parities():
    seen, lengths = set(), set()
    for case in T.of_group("A2"):
        b = T.built(case)
        cut, tail = b.notes["cut"], b.notes["tail"]
        n = len(b.data)
        assert n == cut + T.K_ROUND + tail and 2 <= tail <= 126 and cut % 4096 == 0
        partial = b.data[cut + T.K_ROUND:]
        pairs = tail // 2
        assert (partial[:2 * pairs] == 10).all()
        if tail % 2:
            assert (partial[-1] == 10) == b.final_newline
        if case.id.startswith("A2-inside"):
            assert not (b.data[cut - 90:cut + T.K_ROUND] == 10).any()        # the whole round inside one line: no result held
        else:
            assert b.data[cut - 1] == 10 and int((b.data[cut:cut + T.K_ROUND] == 10).sum()) == 2
        seen.add((case.id.split("-")[1], tail % 2, b.final_newline))
        lengths.add(tail)
    assert seen == {(a, p, f) for a in ("inside", "fresh") for (p, f) in ((0, True), (1, True), (1, False))}
    # (31 - 2 KB: a lane that holds 0 or 4 result bits and meets eight pairs and more has 28 in the register in front of a pair)
    assert lengths >= {2, 3, 125, 126} and sum(1 for p in T.A2_PAIRS if p >= 8) >= 3


def test_a3_straddling_lines_end_on_both_bytes_of_a_pair():
    (case,) = T.of_group("A3")
    b = T.built(case)
    rep, o = table()
    nl = newline_offsets(b)
    want = T.expected(case, o)
    seen = set()
    for at, boundary, extra, e, behind in b.notes["placed"]:
        end = int(nl[at])
        start = int(nl[at - 1]) + 1 if at else 0
        assert boundary % 4096 == 0 and start == boundary - 60 and end == boundary + extra + e
        two_in_pair = end % 2 == 0 and b.data[end + 1] == 10
        assert two_in_pair == (e % 2 == 0 and behind == b"")
        for stripe in (512, 4096):
            crossed = end // stripe - start // stripe
            seen.add((stripe, min(crossed, 3), end % 2, len(behind), int(want[at])))
    for stripe in (512, 4096):
        for crossed in (1, 3):
            for parity in (0, 1):
                for behind in (0, 1):
                    for verdict in (0, 1):
                        assert (stripe, crossed, parity, behind, verdict) in seen, (stripe, crossed, parity, behind, verdict)


def test_a4_shared_wide_word_holds_0_2_and_30_bits_of_the_first_workgroup():
    seen = set()
    for case in T.of_group("A4"):
        b = T.built(case)
        k, fresh = b.notes["lines_mod_16"], b.notes["fresh"]
        assert T.A4_CUT < len(b.data) <= 2 * T.A4_CUT, "two workgroups at stripe 512"
        in_front = int((b.data[:T.A4_CUT] == 10).sum())
        assert in_front % 16 == k and (b.data[T.A4_CUT - 1] == 10) == fresh
        nl = newline_offsets(b)
        s = b.notes["straddler"]
        assert s in b.escaping and (int(nl[s]) == T.A4_CUT - 1 if fresh else int(nl[s - 1]) < T.A4_CUT < int(nl[s]))
        seen.add((2 * k, fresh))
    assert seen == {(bits, f) for bits in (0, 2, 30) for f in (True, False)}


def test_a5_escaping_lines_lie_beyond_every_window():
    (case,) = T.of_group("A5")
    b = T.built(case)
    rep, o = table()
    want = T.expected(case, o)
    assert len(b.data) <= 1 << 20 and len(b.data) > T.A4_CUT
    nl = newline_offsets(b)
    for stripe in (512, 4096):
        wg_bytes = T.K_THREADS * stripe
        beyond = set()
        for wg in range((len(b.data) + wg_bytes - 1) // wg_bytes):
            first_line = int(np.searchsorted(nl, wg * wg_bytes))           # line ends in front of the workgroup's first byte
            last_line = int(np.searchsorted(nl, min((wg + 1) * wg_bytes, len(b.data)) - 1))
            assert (2 * last_line >> 5) - (2 * first_line >> 5) >= 16000 > T.WINDOW_WORDS_MAX
            for i in b.escaping:
                if first_line <= i <= last_line and (2 * int(i) >> 5) - (2 * first_line >> 5) >= T.WINDOW_WORDS_MAX:
                    beyond.add((wg, int(want[i])))
        assert beyond == {(wg, v) for wg in range(1 if stripe == 4096 else 2) for v in (0, 1)}, (stripe, beyond)


def test_b_cases_reach_the_split_edges():
    sizes = set()
    for case in T.of_group("B1"):
        n = len(T.built(case).idx)
        sizes.add(((n + 31) // 32, n % 32))
    assert sizes == {(w, m) for w in (1, 255, 256, 257) for m in (1, 31, 0)}
    totals = {}
    for case in T.of_group("B2"):
        b = T.built(case)
        lo, hi = b.notes["block"]
        assert lo % T.BLOCK_LINES == 0 and hi - lo == T.BLOCK_LINES and lo // T.BLOCK_LINES < T.SPLIT_GRID_MAX
        assert len(b.idx) == T.B2_LINES and ((b.escaping >= lo) & (b.escaping < hi)).all()
        per_lane = np.bincount((b.escaping - lo) // 32, minlength=T.SPLIT_BLOCK_WORDS)
        totals[len(b.escaping)] = int(per_lane.max())
    # eight lines per lane and round of the append: 2048 after the first round (no flush: not above kFlushAt), the 2049th in a second
    assert totals == {T.SPLIT_FLUSH_AT: 8, T.SPLIT_FLUSH_AT + 1: 9, T.BLOCK_LINES: 32}
    assert T.SPLIT_FLUSH_AT < T.SPLIT_FLUSH_AT + 1 <= T.list_capacity(T.B2_LINES) < T.BLOCK_LINES
    (case,) = T.of_group("B3")
    b = T.built(case)
    words = (len(b.idx) + 31) // 32
    assert T.SPLIT_GRID_MAX * T.SPLIT_BLOCK_WORDS < words <= 2 * T.SPLIT_GRID_MAX * T.SPLIT_BLOCK_WORDS, "two turns"
    assert (17 << 20) <= len(b.data) <= (34 << 20)
    assert (b.escaping < T.SPLIT_TURN_LINES).sum() >= 4 and (b.escaping >= T.SPLIT_TURN_LINES).sum() >= 4
    assert T.SPLIT_TURN_LINES - 1 in b.escaping and T.SPLIT_TURN_LINES in b.escaping and 0 in b.escaping and len(b.idx) - 1 in b.escaping


def test_c_totals_lie_on_both_sides_of_both_caps():
    seen = set()
    for case in T.of_group("C"):
        b = T.built(case)
        n = len(b.idx)
        cap = T.list_capacity(n)
        words = (n + 31) // 32
        assert n <= 65536 if cap == T.LIST_FLOOR else (n == 131072 and cap == words // 2 > T.LIST_FLOOR)
        seen.add((cap, len(b.escaping) - cap))
    assert seen == {(cap, d) for cap in (1024, 2048) for d in (-1, 0, 1)}


@pytest.mark.parametrize("group", ("D", "E"))
def test_line_starts_of_the_escaping_lines(group):
    rep, o = table()
    finals = set()
    for case in T.of_group(group):
        b = T.built(case)
        at = b.notes["at"]
        starts = T.line_starts(b.data)
        n = len(b.data)
        finals.add(b.final_newline)
        assert len(starts) == len(b.idx)

        def front(name):                                     # offset of the '\n' in front of the named line
            return int(starts[at[name]]) - 1
        assert at["line 0"] == 0 and 0 in b.escaping
        for residue in T.D_RESIDUES:
            assert front("mod 64 = %d" % residue) % 64 == residue
        for stripe in (512, 4096):
            assert front("behind stripe %d" % stripe) % stripe == stripe - 1
        for nth in (1, 8, 16):
            p = front("newline %d of its 16 bytes" % nth)
            chunk = b.data[p - p % 16:p - p % 16 + 16]
            assert int((chunk[:p % 16 + 1] == 10).sum()) == nth == p % 16 + 1
            assert (b.data[p - 64:p] == 10).all()            # dense: the 64-byte count in front of it is 64
        assert 16 <= n - int(starts[at["less than 64 from the end"]]) < 64 and n - int(starts[at["less than 16 from the end"]]) < 16
        assert at["less than 16 from the end"] == len(b.idx) - 1
        named = [v for k, v in at.items() if not k.startswith("no line starts") and not k.startswith("NUL")]
        assert set(named) <= set(int(i) for i in b.escaping) and at["NUL in front"] not in b.escaping and at["NUL inside"] not in b.escaping
        want = T.expected(case, o)
        assert want[at["NUL inside"]] == 0 and want[at["NUL in front"]] == 0
        if group == "E":
            esc_set = set(int(i) for i in b.escaping)
            for stripe in (512, 4096):
                owner = starts // stripe                      # the stripe every line starts in
                empty = at["no line starts %d" % stripe] // stripe
                assert empty * stripe == at["no line starts %d" % stripe] and not (owner == empty).any()
                for name, pick in (("first", 0), ("last", -1)):
                    i = at["%s of stripe %d" % (name, stripe)]
                    mine = np.nonzero(owner == owner[i])[0]
                    assert len(mine) > 2 and int(mine[pick]) == i and [int(k) for k in mine if int(k) in esc_set] == [i]
    assert finals == {True, False}
