"""The automata on the limit of every table form (table_edge_cases.py), on the CPU: the library itself must place each case where
the case set says - form name, states, classes, pair columns, the fit expression against its constant - and its neighbour on the
next form; then the case's text is replayed through the PACKED table - the device image's entries restated from pack.cpp: 16-bit
row byte offsets, interleaved copies, the '\\n' column - the way the kernels address it (table_engines.hpp), against the expected
verdicts.  The replay records the rows it visits: every row must be visited, and the row at the highest offset left through an
accepted and through a rejected line.  Last, the proof that the texts would notice a bug: the replay again with the next-row field
truncated to 15 bits, and with the highest row aliased to row 0 - some verdict of every at-limit case must change."""
import re

import numpy as np
import pytest

import roaringregex_amd as rr
import table_edge_cases as T
from program_replay import DfaReplay

TRUNCATE15, ALIAS_TOP = "next-row field truncated to 15 bits", "highest row aliased to row 0"


class Walk:
    """What one replayed line did: its verdict, and the rows it took a transition out of."""

    def __init__(self):
        self.verdict, self.rows = 0, set()


class PackedTable:
    """The part the two packed forms share: a flat array of 32-bit entries, low 16 bits = byte offset of the next row (of copy 0;
    copy k adds 4 k), and the corruption applied to every entry as it is read."""

    def corrupt(self, how):
        assert how in (TRUNCATE15, ALIAS_TOP)
        self.how = how
        return self

    def read(self, byte_off):
        """The entry at a byte offset of the table; an address outside it reads 0, as LDS behind the table would (the dead row)."""
        i = byte_off >> 2
        e = int(self.flat[i]) if 0 <= i < len(self.flat) else 0
        if self.how == TRUNCATE15:
            e = (e & 0xffff0000) | (e & 0x7fff)
        elif self.how == ALIAS_TOP and (e & 0xffff) == self.top_off:
            e &= 0xffff0000
        return e

    @property
    def top_off(self):
        return (self.nrows - 1) * self.row_bytes

    def at_start(self):
        e = self.start_off
        if self.how == TRUNCATE15:
            e &= 0x7fff
        elif self.how == ALIAS_TOP and e == self.top_off:
            e = 0
        return e


class PackedLineTable(PackedTable):
    """pack_dfa_tables' line table (wide: 129 byte columns, R interleaved copies; classed: ncls + 1 columns, an odd stride) and
    pack_items' items table (131 columns, 129 = END OF ITEM), stepped as LineDfaEngine::step does: entry = table[(e & 0xffff) +
    (column << (2 + log2 R))], byte 2 = a line ended, byte 3 = its verdict."""

    def __init__(self, dfa_words, wide, items=False):
        d = DfaReplay(dfa_words)
        D, K = d.nstates, d.ncls
        nxt, cls, acc = d.next.astype(np.int64), d.cls.astype(np.int64), d.acc.astype(np.int64)
        self.how, self.nrows, self.items, self.wide = None, D, items, wide or items
        if items:
            stride, R = 131, T.items_copies(D)
        elif wide:
            stride, R = 129, T.wide_copies(D)
        else:
            stride, R = (K + 1) | 1, 1
        self.R, self.row_bytes = R, stride * 4 * R
        assert (D - 1) * self.row_bytes + 4 * (R - 1) <= 0xffff, "the highest row's offset does not fit 16 bits"
        tab = np.zeros((D, stride), dtype=np.int64)
        end_entry = d.start * self.row_bytes | 1 << 16 | acc << 24
        if items:
            for c in range(129):
                nx = nxt[:, cls[c]]
                tab[:, c] = nx * self.row_bytes | (acc[nx] * 0x80) << 16
            tab[:, 129] = end_entry
            self.end_col = 129
        elif wide:
            for c in range(129):
                tab[:, c] = nxt[:, cls[c]] * self.row_bytes
            tab[:, 10] = end_entry
            self.end_col = 10
        else:
            tab[:, :K] = nxt * self.row_bytes
            tab[:, K] = end_entry
            self.end_col, self.cls = K, cls
        self.flat = (tab.reshape(-1, 1) + 4 * np.arange(R).reshape(1, -1)).reshape(-1)        # copy k of entry i at i * R + k
        self.start_off = d.start * self.row_bytes
        self.shift = 2 + R.bit_length() - 1

    def column(self, c):
        return min(c, 128) if self.wide else int(self.cls[c])

    def walk(self, line, lead=0):
        w, e = Walk(), self.at_start()
        for col in [self.column(c) for c in line] + [self.end_col]:
            row = (e & 0xffff) // self.row_bytes
            w.rows.add(row)
            e = self.read((e & 0xffff) + (col << self.shift))
        assert self.how or (e >> 16) & 0xff == 1, "the '\\n' column ends one line"
        w.verdict = (e >> 24) & 1
        return w


class PackedDfa2Table(PackedTable):
    """pack_dfa2's stride-2 table (rows of ncols | 1 entries, R2 copies; P[c1][c2] = the pair's column byte offset), stepped as
    Dfa2T::step2 does: entry = T2[(e & 0xffff) + P[c1][c2]], byte 2 = lines ended in the pair, byte 3 = their verdicts (oldest
    highest).  The items form has 129 codes, 128 = END OF ITEM.  Bytes >= 0x80 are stepped as 0x00."""

    def __init__(self, words, items=False):
        w = np.asarray(words, dtype=np.int64)
        D, C, start = int(w[0]), int(w[1]), int(w[2])
        self.dim = int(w[4]) if items else 128
        o = 5 if items else 4
        assert self.dim == (129 if items else 128)
        pair_col = w[o:o + self.dim * self.dim].reshape(self.dim, self.dim)
        next2 = w[o + self.dim * self.dim:].reshape(D, C)
        s2, R = C | 1, T.dfa2_copies(D, C)
        self.how, self.nrows, self.R, self.row_bytes, self.end = None, D, R, s2 * 4 * R, (128 if items else 10)
        assert (D - 1) * self.row_bytes + 4 * (R - 1) <= 0xffff, "the highest row's offset does not fit 16 bits"
        tab = np.zeros((D, s2), dtype=np.int64)
        tab[:, :C] = (next2 & 0xffff) * self.row_bytes | (next2 & 0xffff0000)
        self.flat = (tab.reshape(-1, 1) + 4 * np.arange(R).reshape(1, -1)).reshape(-1)
        self.P = pair_col * 4 * R
        self.start_off = start * self.row_bytes

    def walk(self, line, lead=0):
        """The line behind `lead` (0 / 1) terminators, so that it begins on the first / second code of a pair."""
        seq = [self.end] * lead + [c if c < 128 else 0 for c in line] + [self.end]
        if len(seq) % 2:
            seq.append(self.end)
        w, e, out = Walk(), self.at_start(), []
        for i in range(0, len(seq), 2):
            row = (e & 0xffff) // self.row_bytes
            w.rows.add(row)
            e = self.read((e & 0xffff) + int(self.P[seq[i], seq[i + 1]]))
            lines, verdicts = (e >> 16) & 0xff, e >> 24
            out += [(verdicts >> (lines - 1 - k)) & 1 for k in range(lines)]
        assert self.how or len(out) in (lead + 1, lead + 2), (len(out), lead)
        w.verdict = out[lead] if len(out) > lead else 0
        return w


def program_kinds(case):
    """(byte-stride program kind, stride-2 program kind) of the table a case is about."""
    if case.table == "contains":
        return rr.PROGRAM_CONTAINS_DFA, rr.PROGRAM_CONTAINS_DFA2
    return rr.ENGINE_DFA, rr.ENGINE_DFA2


def packed_tables(case, r):
    """[(name, PackedTable factory)] - every LDS form of the case's table that the kernels read with 16-bit row offsets."""
    dfa_kind, dfa2_kind = program_kinds(case)
    dfa = r.program(dfa_kind)
    out = []
    if case.table in ("match", "contains"):
        form = r.contains_engine_name if case.table == "contains" else r.engine_name
        if form == "dfa-stride2-table":
            out.append(("stride-2", lambda: PackedDfa2Table(r.program(dfa2_kind))))
        elif form in ("dfa-wide-table", "dfa-classed-table"):
            out.append((form, lambda: PackedLineTable(dfa, wide=form == "dfa-wide-table")))
    elif case.table == "items":
        if int(dfa[0]) * 131 * 4 * T.items_copies(int(dfa[0])) <= 65535:
            out.append(("byte-stride items", lambda: PackedLineTable(dfa, wide=True, items=True)))
        if r.program(rr.PROGRAM_DFA2_ITEMS) is not None:
            out.append(("stride-2 items", lambda: PackedDfa2Table(r.program(rr.PROGRAM_DFA2_ITEMS), items=True)))
    return out


def replay(table, distinct, leads):
    """{(line index, lead): Walk}"""
    return {(i, lead): table.walk(ln, lead) for i, ln in enumerate(distinct) for lead in leads}


def regex_of(case):
    return rr.RRegex(case.pattern, case.engine)


def shape(pattern):
    """The family of a pattern: its text with the last repetition count, or the number of literals, left out."""
    if pattern.startswith(T.ALNUM):
        return "literal" if len(pattern) % 62 else "alnum"
    return re.sub(r"\d+\}$", "N}", pattern)


IDS = [c.id for c in T.CASES]


# ------------------------------------------------------------------------------------------------------------ boundaries
@pytest.mark.parametrize("case_id", IDS)
def test_the_library_places_the_case_where_the_case_set_says(case_id):
    case = T.BY_ID[case_id]
    r = regex_of(case)
    dfa_kind, dfa2_kind = program_kinds(case)
    dfa = r.program(dfa_kind)
    D, K = int(dfa[0]), int(dfa[1])
    at = case.side == "at"
    if case.table in ("match", "contains"):
        form = r.contains_engine_name if case.table == "contains" else r.engine_name
        assert form == case.form, (case_id, form)
        if case.table == "contains":
            assert r.contains_states == D
        if case.limit.startswith("nstates * 516"):
            copies = T.wide_copies(D)
            assert case.limit.endswith("R = %d" % copies) and D * 516 * copies == case.value <= 65536, (case_id, D, copies)
            # at: one state more halves the copies; past: the state that did
            assert ((D + 1) * 516 * copies > 65536) == at and (D * 516 * 2 * copies > 65536), (case_id, D, copies)
            assert at or T.wide_copies(D - 1) == 2 * copies
        elif case.limit == "nstates <= 127":
            assert D == case.value and (D <= T.WIDE_MAX_STATES) == at and D in (127, 128), (case_id, D)
        elif case.limit.startswith("nstates * (ncls"):
            assert T.classed_entries(dfa) == case.value and (case.value <= T.CLASSED_MAX_ENTRIES) == at, (case_id, D, K)
        else:
            assert case.limit.startswith("nstates * (ncols")
            if form == "dfa-stride2-table":
                d2 = r.program(dfa2_kind)
                assert int(d2[0]) == D and T.dfa2_bytes(d2) == case.value <= T.DFA2_MAX_TABLE and case.side in ("at", "inside"), (case_id, d2[:2])
            else:                                   # no stride-2 program: the size comes from the at-limit neighbour's column count
                assert r.program(dfa2_kind) is None and case.side == "past" and case.value > T.DFA2_MAX_TABLE
                assert case.value % (D * 4) == 0 and (case.value // (D * 4)) & 1, (case_id, D)
    elif case.table == "items":
        assert r.engine_name == "dfa-stride2-table" or case.id == "items2-past-a{1535}"
        items2 = r.program(rr.PROGRAM_DFA2_ITEMS)
        if case.limit.startswith("nstates * 131"):
            assert D * 131 * 4 * T.items_copies(D) == case.value and (case.value <= 65535) == at and D == (125 if at else 126), (case_id, D)
            assert items2 is not None                # (the stride-2 items form serves both; the test switches it off)
        else:
            assert (items2 is not None) == at
            size = T.dfa2_bytes(items2) if at else D * 7 * 4
            assert size == case.value and (size <= T.DFA2_MAX_TABLE) == at, (case_id, size)
            assert D * 131 * 4 > 65535               # (no byte-stride items table either way)
    elif case.table == "plain":
        assert r.engine_name == "dfa-global-table"   # (the LINE table: too large for any LDS form - the plain table is another matter)
        size = T.plain_lds_bytes(dfa)
        assert size == case.value and (size <= T.PLAIN_LDS_BUDGET) == at and (case.form == "lds") == at, (case_id, size)
        contains = r.program(rr.PROGRAM_CONTAINS_DFA)    # (a{13054} has none: its forward search automaton passes the state budget)
        assert (contains is None) == case.pattern.startswith("a{") and (contains is None or T.plain_lds_bytes(contains) == size), case_id
    else:
        st, an = r.program(rr.PROGRAM_SEARCH_STARTS), r.program(rr.PROGRAM_SEARCH_ANCHORED)
        size = T.plain_lds_bytes(st) + T.plain_lds_bytes(an)
        assert size == case.value and (size <= T.PLAIN_LDS_BUDGET) == at and (case.form == "lds") == at, (case_id, size)
    # the families: a{n} and a{1,n} have n + 2 states, (ab|cd|ef){n} 4 n + 2, the literal of 62 k bytes 62 k + 2
    unit = 2 if case.pattern.startswith("(") else 62 if shape(case.pattern) == "alnum" else 1
    assert D == (2 if unit == 2 else 1) * len(case.members[0]) + 2, (case_id, D)
    if at:                                          # the largest of its family: the case one repetition further is in the set, on the other side
        beyond = [c for c in T.CASES if (c.table, c.limit.split(",")[0], c.side) == (case.table, case.limit.split(",")[0], "past") and
                  len(c.members[0]) == len(case.members[0]) + unit and shape(c.pattern) == shape(case.pattern)]
        assert len(beyond) == 1 and beyond[0].engine == case.engine, (case_id, [c.id for c in beyond])


def test_the_plain_limit_is_the_rounded_size():
    """The two plain tables of a{6499} and a{6500} together are below 64 KiB by plain_table_bytes and beyond it by the size the
    kernels compare (both arrays rounded up to 16 bytes): the pair at the limit is found with the latter."""
    r = rr.RRegex("a{6499}")
    st, an = r.program(rr.PROGRAM_SEARCH_STARTS), r.program(rr.PROGRAM_SEARCH_ANCHORED)
    assert T.plain_table_bytes(st) + T.plain_table_bytes(an) <= 65536 < T.plain_lds_bytes(st) + T.plain_lds_bytes(an)


def test_the_stride2_engine_refuses_the_first_automaton_beyond_its_limit():
    assert len(T.DFA2_REFUSED) == 4
    for p in T.DFA2_REFUSED:
        with pytest.raises(rr.RRegexError, match="too large"):
            rr.RRegex(p, rr.ENGINE_DFA2)
    for c in T.cases("match", "at") + T.cases("match", "inside"):
        if c.form == "dfa-stride2-table":
            assert rr.RRegex(c.pattern, rr.ENGINE_DFA2).engine_name == "dfa-stride2-table", c.id


# ------------------------------------------------------------------------------------------------------------ texts
REPLAYED = [c.id for c in T.CASES if c.table in ("match", "contains", "items")]


@pytest.mark.parametrize("case_id", REPLAYED)
def test_the_text_follows_the_text_rule(case_id):
    case = T.BY_ID[case_id]
    distinct, idx = T.build_lines(case_id)
    starts, lens = T.line_starts(distinct, idx)
    total = int(starts[-1] + lens[-1] + 1)
    assert T.WG_BYTES + 512 < total <= (1 << 20) and (total + 511) // 512 > T.WG_STRIPES
    m = case.members[0]
    assert b"" in distinct and all(bytes([c]) in distinct for c in set(b"".join(case.members)))
    for mem in case.members:
        for ln in (mem, mem[:-1], mem + mem[-1:], mem[:-1] + b"\x00", mem[:-1] + b"\xc3", mem[:-1] + T.other_byte(case, mem)):
            assert ln in distinct, (case_id, len(ln))
    mi = distinct.index(m)
    s = starts[idx == mi]
    assert {int(x) % 2 for x in s} == {0, 1}, "the member begins on both bytes of a pair"
    if len(m) >= 2:
        assert ((s // 512) != ((s + len(m) - 1) // 512)).any(), "a member across a stripe end"
        assert ((s < T.WG_BYTES) & (s + len(m) > T.WG_BYTES)).any(), "a member across the workgroup cut"
    clean, cidx = T.build_lines(case_id, high=False)
    assert not any(c >= 0x80 for ln in clean for c in ln) and len(clean) < len(distinct)


# ------------------------------------------------------------------------------------------------------------ replay
@pytest.mark.parametrize("case_id", REPLAYED)
def test_replay_of_the_packed_table(case_id):
    case = T.BY_ID[case_id]
    r = regex_of(case)
    distinct, idx = T.build_lines(case_id)
    data, want = T.expected(case_id)
    per_line = T.closed_form(case, distinct)
    assert (per_line[idx] == want).all() and 0 < want.sum() < len(want)
    tables = packed_tables(case, r)
    if case.form == "dfa-global-table" or case.form == "lane per item" and not tables:
        # a table in HBM/L2 holds 24-bit entry indices and a plain table 16-bit state numbers: the plain program, row by row
        d = DfaReplay(r.program(program_kinds(case)[0]))
        seen = set()
        for ln, v in zip(distinct, per_line):
            st = d.start
            for c in ln:
                seen.add(st)
                st = int(d.next[st, d.cls[c]])
            seen.add(st)
            assert int(d.acc[st]) == int(v), (case_id, len(ln))
        if case.table == "contains":
            assert not (d.next[1:] == 0).any(), case_id
            seen.add(0)
        assert seen == set(range(d.nstates)), (case_id, "rows never visited", sorted(set(range(d.nstates)) - seen)[:5])
        return
    assert tables, case_id
    checked = 0
    for name, make in tables:
        table = make()
        leads = (0, 1) if isinstance(table, PackedDfa2Table) else (0,)
        walks = replay(table, distinct, leads)
        for (i, lead), w in walks.items():
            assert w.verdict == per_line[i], (case_id, name, "line", i, len(distinct[i]), "lead", lead)
        rows = set().union(*(w.rows for w in walks.values()))
        if case.table == "contains":                # no text leads a contains table into row 0 (the row of the lanes that wait for their '\n')
            assert not (DfaReplay(r.program(rr.PROGRAM_CONTAINS_DFA)).next[1:] == 0).any(), case_id
            rows.add(0)
        assert rows == set(range(table.nrows)), (case_id, name, "rows never visited", sorted(set(range(table.nrows)) - rows)[:5])
        top = table.nrows - 1

        def left(row):
            return {int(per_line[i]) for (i, lead), w in walks.items() if row in w.rows}
        if case.table == "contains":                # its highest row is the accepting row that no byte leaves: accepted lines only;
            assert left(top) == {1} and left(top - 1) == {0, 1}, (case_id, name, left(top), left(top - 1))      # the row below it: both
        else:
            assert left(top) == {0, 1}, (case_id, name, "the highest row is left through verdicts", left(top))
        if case.side != "at" or table.top_off + 4 * (table.R - 1) < 0x8000:      # (a{123}'s stride-2 items table: 8 copies of 125 rows,
            continue                                                              #  far from its limit - the byte-stride one is the case)
        checked += 1
        # sensitivity: with either corruption some verdict of this text changes
        for how in (TRUNCATE15, ALIAS_TOP):
            bad = replay(make().corrupt(how), distinct, leads)
            changed = [k for k in walks if bad[k].verdict != walks[k].verdict]
            assert changed, (case_id, name, how, "no verdict of the text changes")
    assert checked == (case.side == "at"), (case_id, "tables whose sensitivity was checked", checked)


@pytest.mark.parametrize("case_id", [c.id for c in T.cases("plain")])
def test_the_items_of_a_plain_table_case_walk_every_row(case_id):
    """The plain tables hold 16-bit state NUMBERS (no offsets to truncate): the program row by row - the match table on the whole item,
    the contains table where the pattern has one - gives the expected verdicts and meets every row."""
    case = T.BY_ID[case_id]
    r = regex_of(case)
    distinct = T.distinct_lines(case)
    for kind, per_line in ((rr.ENGINE_DFA, T.closed_form(case, distinct)), (rr.PROGRAM_CONTAINS_DFA, None)):
        words = r.program(kind)
        if words is None:
            assert kind == rr.PROGRAM_CONTAINS_DFA and case.pattern.startswith("a{")
            continue
        if per_line is None:
            per_line = T.contains_expected(case, distinct)
        d = DfaReplay(words)
        nxt, cls, seen = d.next.tolist(), d.cls.tolist(), set()
        for ln, v in zip(distinct, per_line):
            st = d.start
            for c in ln:
                seen.add(st)
                st = nxt[st][cls[c]]
            seen.add(st)
            assert int(d.acc[st]) == int(v), (case_id, kind, len(ln))
        if kind == rr.PROGRAM_CONTAINS_DFA:
            assert not (d.next[1:] == 0).any()
            seen.add(0)
        assert seen == set(range(d.nstates)), (case_id, kind, sorted(set(range(d.nstates)) - seen)[:5])
