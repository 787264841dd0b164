"""The corpora of tests/search_cases.py, checked on the host: (1) for every builder and pattern that tests/test_search_corpus_gpu.py
uses, the expectation composed from the oracle's brute force per cell equals the replay of the search tables on the whole line
(SearchReplay, and SearchLine2Replay with the line on either byte of a pair) - the separator argument, proved per pattern instead of
assumed; (2) every case puts its features where its name says: at the stated offset modulo 2, 4, 16, 256 and 16384, with the stated
number of lines per chunk, with lines that match and lines that do not.  Nothing is skipped or filtered: the builders assert that every
requested placement exists (CaseBuilder.finish, verify_placements)."""
import random

import numpy as np
import pytest

import roaringregex_amd as rr
import search_cases as sc
from patterns import EMAIL
from program_replay import SearchLine2Replay, SearchReplay
from pyoracle import OracleRegex

_REPLAYS = {}


def replays(pattern, anchored=True):
    key = (pattern, anchored)
    if key not in _REPLAYS:
        r = rr.RRegex(pattern)
        if not anchored:
            r.set_search_anchored(False)
        rev = r.program(rr.PROGRAM_SEARCH_REV)
        l2 = r.program(rr.PROGRAM_SEARCH_LINE2)
        _REPLAYS[key] = (SearchReplay(r.program(rr.PROGRAM_SEARCH_FWD), rev), SearchLine2Replay(l2, rev) if l2 is not None else None)
    return _REPLAYS[key]


def replay_agrees(pattern, case, picks, what, line2_below=3000):
    """The composed expectation of the lines `picks` against the table replays on the whole line."""
    rep, l2 = replays(pattern)
    seen = set()
    for i in picks:
        ln = case.lines[i]
        if ln in seen:
            continue
        seen.add(ln)
        assert rep.search(ln) == tuple(case.first_want[i]), (what, pattern, i, ln[:60])
        assert rep.search_all(ln) == list(case.all_want[i]), (what, pattern, i, ln[:60])
        if l2 is not None and len(ln) < line2_below:
            for lead in (0, 1):
                assert l2.search(ln, lead) == tuple(case.first_want[i]), (what, pattern, i, lead, ln[:60])
                assert l2.search_all(ln, lead) == list(case.all_want[i]), (what, pattern, i, lead, ln[:60])
    return len(seen)


def sample(case, n, below, seed=3, always=()):
    rng = random.Random(seed)
    short = [i for i, ln in enumerate(case.lines) if len(ln) < below]
    return sorted(set(rng.sample(short, min(n, len(short)))) | {i for i in always if len(case.lines[i]) < below})


def matched_and_unmatched(case):
    has = [bool(w) for w in case.all_want]
    assert any(has) and not all(has), "lines with and without a match"
    assert [f[1] >= 0 for f in case.first_want] == has
    assert all(w[0] == f for w, f in zip(case.all_want, case.first_want) if w)


def test_cells_are_what_their_kind_says():
    for pattern, sp in sc.SPECS.items():
        cells, o = sc.Cells.of(pattern), OracleRegex(pattern)
        every = sp.lead + sp.inner + sp.miss + (sp.sized or [])
        st, en = o.search_lines(b"\n".join(every) + b"\n")
        for c, s, e in zip(every, st.tolist(), en.tolist()):
            ms = cells.matches(c)
            assert (ms[0] if ms else (-1, -1)) == (s, e), (pattern, c, "all matches begin with the first match")
            assert len(c) <= sc.MAX_CELL
        assert all(cells.matches(c)[0][0] == 0 for c in sp.lead) and all(cells.matches(c)[0][0] > 0 for c in sp.inner), pattern
        assert not any(cells.matches(c) for c in sp.miss), pattern
        assert sp.sep not in b"".join(every)
        if sp.sized:
            assert sorted((cells.matches(c)[0][1] - cells.matches(c)[0][0]) % 4 for c in sp.sized) == [0, 1, 2, 3], pattern
        # no match contains or spans the separator: cells glued by one separator give the cells' matches
        rng = random.Random(len(pattern))
        parts = []
        for c in rng.sample(every * 3, 2 * len(every)):
            parts += [sc.cell(c), sc.gap(rng.randint(1, 3), sp.sep)]
        case = sc.assemble(pattern, [parts, parts[::-1][1:]], True)
        assert replay_agrees(pattern, case, (0, 1), "glued cells") == 2
        if pattern in (EMAIL, sc.GLOBAL_FORM):               # and the oracle's own answer on whole lines
            sc._oracle_confirms_search(pattern, case.lines, first=case.first_want, every=case.all_want, starts_per_match=4)


@pytest.mark.parametrize("pattern,step", [("ab+c", 1), ("ab+c", 5), (sc.GLOBAL_FORM, 5)])
def test_residue_case(pattern, step):
    case = sc.residue_case(pattern, step=step)
    matched_and_unmatched(case)
    by = {}
    for p in case.placed:
        by.setdefault(p["name"], []).append(p)
    lane_offsets = {p["at"] % sc.LANE for p in by["line_start"]}
    assert {0, 1, 15, 16, 255} <= lane_offsets and (step > 1 or lane_offsets == set(range(256)))
    assert {0, 63} <= {p["at"] % sc.CHUNK // sc.LANE for p in by["line_start"] if p["modulus"] == sc.CHUNK}
    assert {p["at"] % sc.CHUNK for p in by["newline"]} >= {sc.CHUNK - 1} and {p["at"] % sc.LANE for p in by["newline"]} == {sc.LANE - 1}
    ends = [p for p in by["match_end"] if "behind_lane" not in p and "crosses" not in p]
    assert {p["at"] % sc.WORD for p in ends} == set(range(16)) and {p["at"] % sc.PAIR for p in ends} == {0, 1}
    assert {0, 15} <= {p["at"] % sc.LANE // sc.WORD for p in ends}, "first and last event word of a lane"
    assert step > 1 or {p["at"] % sc.LANE for p in ends} == set(range(256))
    assert {p["at"] % sc.WALK for p in by["match_start"]} == set(range(4))
    for p in by["match_end"]:
        if "crosses" in p:                                   # the match starts before the boundary, in a line that began before it
            i = p["line"]
            s = [s for s, e in case.all_want[i] if e == p["at"] - int(case.starts[i]) + 1][0] + int(case.starts[i])
            assert s // p["crosses"] < p["at"] // p["crosses"] and int(case.starts[i]) // p["crosses"] < p["at"] // p["crosses"], p
    assert sorted(p["behind_lane"] for p in by["match_end"] if "behind_lane" in p) == sorted(2 * sc.FOLLOW_DISTANCES)
    assert {(int(case.starts[p["line"]]) % sc.CHUNK) // sc.LANE for p in by["match_end"] if "behind_lane" in p} == {0, 63}
    for p in by["line_start"]:
        if "follow_hits" in p:                               # so many hits behind the last byte of the line's lane
            i = p["line"]
            last = int(case.starts[i]) | (sc.LANE - 1)
            assert sum(int(case.starts[i]) + e - 1 > last for _, e in case.all_want[i]) == p["follow_hits"]
    assert sorted(p["follow_hits"] for p in by["line_start"] if "follow_hits" in p) == list(sc.FOLLOW_HITS)
    picks = sample(case, 250, 400, always=[p["line"] for p in case.placed if p["modulus"] == sc.CHUNK])
    assert replay_agrees(pattern, case, picks, "residues") > 60
    if step == 1:
        long_ones = [p["line"] for p in by["match_end"] if "behind_lane" in p][:9]
        replay_agrees(pattern, case, long_ones, "followed lines", line2_below=600)


def test_bounded_walk_case():
    case = sc.bounded_walk_case()
    matched_and_unmatched(case)
    assert {(p["tail_as"], p["at"] % sc.WALK) for p in case.placed} == {(k, r) for k in range(17) for r in range(4)}
    assert replay_agrees(sc.BOUNDED, case, [p["line"] for p in case.placed], "bounded walks") == 17


def test_end_of_data_cases():
    pattern = "ab+c"
    base = sc.end_of_data_base(pattern)
    seen = {v: 0 for v in sc.END_VARIANTS}
    residues = set()
    for group in sc.END_LENGTHS:
        for n in group:
            residues.add(n % 16)
            for variant in sc.END_VARIANTS:
                case = sc.end_of_data_case(pattern, base, n, variant)
                if case is None:
                    assert variant == "match_at_end" and n < len(sc.SPECS[pattern].lead[0]), "only a match that does not fit n bytes may be missing"
                    continue
                seen[variant] += 1
                assert len(case.data) == n, (n, variant)
                if variant == "final_newline":
                    assert case.data[-1] == 10
                if variant in ("match_at_end", "open_unmatched"):
                    assert case.data[-1] != 10
                if n < 300 or n % 5 == 0:
                    replay_agrees(pattern, case, range(max(0, len(case.lines) - 4), len(case.lines)), (n, variant))
    assert residues == set(range(16)) and all(v >= 83 for v in seen.values())
    whole = sc.assemble(pattern, base, True)
    matched_and_unmatched(whole)
    replay_agrees(pattern, whole, sample(whole, 150, 100), "base")


@pytest.mark.parametrize("pattern", ["ab+c", EMAIL, sc.GLOBAL_FORM])
def test_staging_cases(pattern):
    case, owned = sc.staging_case(pattern)
    assert owned == [m + d for m in range(128, 2049, 64) for d in (-1, 0, 1, 2)] and len(owned) == 124
    assert len(case.data) < (2 << 20) + (64 << 10)
    matched_and_unmatched(case)
    distinct = {}
    for i, ln in enumerate(case.lines):
        distinct.setdefault(ln, i)
    assert replay_agrees(pattern, case, distinct.values(), "staging") == len(distinct)
    if pattern != "ab+c":
        lines = list(distinct)
        sc._oracle_confirms_search(pattern, lines, first=[case.first_want[distinct[ln]] for ln in lines], every=[case.all_want[distinct[ln]] for ln in lines])
    # the open last line of a chunk crosses into the next with a cell on the boundary; every other one has its match there
    last = [int(np.searchsorted(case.starts, (k + 1) * sc.CHUNK)) - 1 for k in range(len(owned))]
    assert all(int(case.starts[i]) + len(case.lines[i]) > (k + 1) * sc.CHUNK for k, i in enumerate(last))
    assert sum(bool(case.all_want[i]) for i in last) == len(owned) // 2
    third = [bool(w) for w in case.all_want[:126]]
    assert third[:6] == [True, False, False, True, False, False]
    # the padded corpora: the lines of the plain corpus come first, unchanged
    multi, _ = sc.staging_case(pattern, pad="multi")
    assert multi.lines[:len(case.lines)] == case.lines and len(multi.data) < (8 << 20)
    for piece in sc.STAGE_PIECES:
        plain, own = sc.staging_case(pattern, piece, pad="plain")
        assert len(plain.data) <= (8 << 20) and own == [m + d for m in piece for d in (-1, 0, 1, 2)]
        assert not plain.all_want[-1] and b"\n" not in plain.lines[-1] and len(plain.lines[-1]) > 60 * sc.CHUNK
    assert sorted(m for piece in sc.STAGE_PIECES for m in piece) == list(sc.STAGE_MULTIPLES)


@pytest.mark.parametrize("pattern", [sc.LONG, "ab+c"])
def test_packing_cases(pattern):
    for long_walk in (True, False):
        case = sc.packing_case(pattern, long_walk)
        matched_and_unmatched(case)
        assert sorted({p["from_line_start"] for p in case.placed}) == sorted(sc.PACK_OFFSETS)
        assert len(case.data) < (2 << 20)
        for p in case.placed:
            s, e = case.first_want[p["line"]]
            assert e == p["from_line_start"] and (s <= 1 if long_walk else e - s <= sc.MAX_CELL)
            assert len(case.all_want[p["line"]]) >= 3, "further matches follow"
        picks = [p["line"] for p in case.placed if p["from_line_start"] <= 0x8001] + sample(case, 30, 100)
        replay_agrees(pattern, case, picks, "packing", line2_below=100)
    case = sc.packing_case(pattern, True)
    assert any(case.first_want[p["line"]][0] == 0 for p in case.placed) and any(case.first_want[p["line"]][0] == 1 for p in case.placed)


def test_dense_line_and_dense_walks():
    case = sc.dense_line_case()
    assert len(case.lines[1]) > 40 << 10 and len(case.all_want[1]) == 20481 > 2048
    replay_agrees(sc.KEYWORD, case, range(len(case.lines)), "dense line", line2_below=1 << 20)
    for pattern in ("ab+c", sc.KEYWORD):
        case = sc.dense_walks_case(pattern)
        matched_and_unmatched(case)
        per_chunk = np.bincount(case.starts // sc.CHUNK)
        assert per_chunk.max() > 2048 and len(case.data) < (1 << 20)
        walks = sum(1 for w in case.all_want for k, (s, e) in enumerate(w) if s > (w[k - 1][1] if k else 0))
        assert walks > 128 * (len(case.data) // sc.CHUNK), "more walk jobs than a wave's pool holds, in every chunk on average"
        # a matching line that starts at a lane's first byte with more lines in front of it in its chunk than any staging array holds: the
        # lane before may not take it for its own (its result goes to memory directly, and a "no match" written behind it would stay)
        ordinal = np.arange(len(case.starts)) - np.searchsorted(case.starts, case.starts // sc.CHUNK * sc.CHUNK)
        assert any(w and s % sc.LANE == 0 and o >= 2048 for w, s, o in zip(case.all_want, case.starts.tolist(), ordinal.tolist())), pattern
        i = case.placed[0]["line"]
        assert all(int(case.starts[j]) % sc.LANE == sc.LANE - 6 and len(case.lines[j]) == sc.LANE - 1 for j in range(i, i + 129))
        replay_agrees(pattern, case, sample(case, 60, 300) + [len(case.lines) - 3, 7501], "dense walks")


def test_odd_byte_cases():
    pattern = "ab+c"
    case = sc.odd_bytes_case(pattern)
    matched_and_unmatched(case)
    for v in sc.ODD_BYTES:
        at = [p["at"] for p in case.placed if p["value"] == v]
        assert {a % sc.WORD for a in at} == set(range(16)) and sc.LANE - 1 in {a % sc.LANE for a in at}
        behind = {a - (int(case.starts[p["line"]]) | (sc.LANE - 1)) for a, p in zip(at, [p for p in case.placed if p["value"] == v])}
        assert len({d % sc.WORD for d in behind if d > 0}) == 16, "in the followed stretch, at every offset of a text word"
    data, fw = case.data, case.first_want
    front = sum(1 for i, (s, e) in enumerate(fw) if e >= 0 and s > 0 and case.lines[i][s - 1] in sc.ODD_BYTES)
    back = sum(1 for i, w in enumerate(case.all_want) for s, e in w if e < len(case.lines[i]) and case.lines[i][e] in sc.ODD_BYTES)
    assert front >= 64 and back >= 64 and data.size < (1 << 20)
    assert replay_agrees(pattern, case, [p["line"] for p in case.placed], "odd bytes") == len(sc.ODD_BYTES) * (3 + 2 + sc.WORD)
    single = sc.single_high_byte_case(pattern)
    matched_and_unmatched(single)
    i = single.placed[0]["line"]
    replay_agrees(pattern, single, [i] + sample(single, 80, 100), "single high byte")


def test_empty_accepting_cases():
    for pattern in sc.EMPTY_ACCEPTING:
        assert OracleRegex(pattern).accepts("")
        rep, l2 = replays(pattern)
        assert l2 is None, "no stripe-wise table: the line-offset path"
        for stripe in (512, 16384):
            for nl in (True, False):
                case = sc.empty_case(stripe, nl)
                assert {len(ln) for ln in case.lines} >= {0, 1, stripe - 1, stripe, stripe + 1, 3 * stripe + 7}
                assert (case.data[-1] == 10) == nl
                for i, ln in enumerate(case.lines):
                    assert rep.search(ln) == case.first_want[i]
                    if len(ln) < 600:
                        assert rep.search_all(ln) == case.all_want[i]
