"""rrx_search_longest_string / rrx_contains_string on the CPU.  The closed forms of long_search_cases.py - the references of the
device test - are pinned, on every case of at most 300 KB, to the sequential SearchLongestReplay of the two program dumps
(RRX_PROGRAM_SEARCH_STARTS, RRX_PROGRAM_SEARCH_ANCHORED: what rrx_search_longest_extents computes for the one-item batch - the
entries' one rule) and, on short random texts, to the brute force over the oracle's whole-string acceptance.  A Python MODEL of the
chunked procedure (chunk maps in walking order, the levels, the down-sweep, the extreme per chunk, its reduction, the forward
windows) gives the same answers - and, run with ONE defect at a time, gets a NAMED device case wrong: the device test's cases can
tell each of these mistakes from the real thing."""
import functools
import random

import pytest

import long_search_cases as S
import roaringregex_amd as rr
from program_replay import DfaReplay
from test_contains_items_lowering import MAX_ITEM, oracle_for
from test_search_longest_items_lowering import SearchLongestReplay, longest_brute_force

CPU_MAX = 300 * 1024


sets, big = S.small_case_sets, S.three_level_cases         # (built once per process)


@functools.lru_cache(maxsize=None)
def tables(pattern):
    r = rr.RRegex(pattern)
    s, a = DfaReplay(r.program(rr.PROGRAM_SEARCH_STARTS)), DfaReplay(r.program(rr.PROGRAM_SEARCH_ANCHORED))
    return s, a, r.accepts_empty


def chunk_route(c):
    """Does the entry take the chunk route for this case (strings.cpp: the threshold and both tables of at most 254 states)?"""
    s, a, _ = tables(c.pattern)
    return c.data.size >= S.SEARCH_FROM and max(s.nstates, a.nstates) <= S.MAX_STATES


def model(c, defect=None):
    s, a, nullable = tables(c.pattern)
    return S.search_model(S.Table(s), S.Table(a), nullable, c.data, c.skew, defect)


def named(set_name, tag):
    hit = [c for c in sets()[set_name] if c.tag == tag]
    assert len(hit) == 1, (set_name, tag, [c.tag for c in sets()[set_name]][:8])
    return hit[0]


def test_the_table_sizes_the_families_were_chosen_for():
    """States of (starts, anchored), from the program dumps: W(k) has k + 3 in both; a{1,300} passes 254 (the hand-over); the URL
    tables are large."""
    want = {S.W(3): (6, 6), S.W(5): (8, 8), S.W(7): (10, 10), S.A300: (3, 302), S.ASTAR: (2, 2), S.XYZ: (2, 5), S.url_pattern(): (156, 90)}
    for p, (ns, na) in want.items():
        s, a, _ = tables(p)
        assert (s.nstates, a.nstates) == (ns, na), p
    # a chunk of a/b text keeps the k residues apart in both directions.  Beside them the anchored table has its dead row alone (the
    # start and the accepting state die on a/b): k + 1 prefix states - W(3) fills exactly the four slots, W(5) and W(7) are flagged.
    # The starts table never dies: its row 0 (unreachable, but a map has it) and its waiting state make k + 2 - flagged for all three.
    for k in (3, 5, 7):
        s, a, _ = tables(S.W(k))
        text = S.L.ab(k, 4 * 256)
        assert (S.L.prefix_distinct(s, text[::-1], 256) == k + 2).all() and (S.L.prefix_distinct(a, text, 256) == k + 1).all(), k
    assert 3 + 1 == S.L.K_LONG_SLOTS
    for p in want:                                            # one column stands for every byte >= 0x80 (lower.hpp: they share class 0)
        for d in tables(p)[:2]:
            assert len(set(d.cls[128:].tolist())) == 1


@pytest.mark.parametrize("name", S.SET_NAMES)
def test_closed_forms_equal_the_sequential_replay(name):
    reps, checked = {}, 0
    for c in sets()[name]:
        if c.data.size > CPU_MAX:
            continue
        rep = reps.get(c.pattern) or reps.setdefault(c.pattern, SearchLongestReplay(rr.RRegex(c.pattern)))
        assert rep.search(c.data.tobytes()) == c.want, c
        checked += 1
    assert checked
    wants = {c.want == S.NONE for c in sets()[name]}
    assert name == "nullable" or wants == {True, False}, "both verdicts in every set (contains_string)"


SMALL_ALPHABETS = {S.W(3): b"abcdz", S.W(5): b"abcd", S.NUMBER: b"0123.z", S.A300: b"az", S.ASTAR: b"az", S.XYZ: b"xyzq", "abcd|c": b"abcdz",
                   "k100|0": b"k10z", S.ABC_B: b"abcz", S.NUM_DOT: b"01.z", S.KNL1: b"k\n1z"}


def test_closed_forms_equal_the_brute_force_at_small_sizes():
    rng = random.Random(2024)
    for p, alphabet in SMALL_ALPHABETS.items():
        fn, o = S.closed_form(p), oracle_for(p)
        seen = set()
        for _ in range(120):
            item = bytes(rng.choice(alphabet) for _ in range(rng.randrange(0, MAX_ITEM + 1)))
            want = longest_brute_force(o, item.replace(b"\n", b"x") if "\n" in p else item)
            assert tuple(fn(item)) == want, (p, item)
            seen.add(want == S.NONE)
        assert p in (S.ASTAR, S.XYZ) or seen == {True, False}, p


@pytest.mark.parametrize("name", S.SET_NAMES)
def test_the_model_of_the_chunked_procedure_gives_the_closed_forms(name):
    checked = 0
    for c in sets()[name]:
        if c.data.size <= CPU_MAX and chunk_route(c):
            assert model(c) == c.want, c
            s, _, nullable = tables(c.pattern)
            assert S.contains_model(S.Table(s), nullable, c.data) == (c.want != S.NONE), c
            checked += 1
    assert checked or name == "hand-over"


def test_the_geometry_the_cases_rely_on():
    """The grids as the source lays them: the backward chunks counted from the end, the forward windows 256 bytes (less the
    address' low bits), then 15 times what has been walked."""
    assert S.forward_windows(0, 100000) == [(0, 256), (256, 3840), (4096, 61440), (65536, 34464)]
    assert S.forward_windows(5, 5000, skew=7)[:2] == [(5, 256 - 12), (5 + 244, 244 * 15)]
    chunk, bounds = S.back_grid(S.POSITION_N)
    assert chunk == 256 and bounds[0] == S.POSITION_N - 256 and len(bounds) == 300
    assert S.long_chunk(S.THREE_LEVELS) == 1024 and (S.THREE_LEVELS + 1023) // 1024 == S.GROUP * S.GROUP + 1
    assert S.SEARCH_FROM - 1 in S.GEOMETRY_LENGTHS and S.SEARCH_FROM + 1 in S.GEOMETRY_LENGTHS


# defect -> the (set, tag) of a device case that the defective model gets wrong
FLIPS = {
    "entries_all_start": ("W(5) positions", "W(5) start at 0, 130 chunks"),
    "downsweep_off_by_one": ("W(5) positions", "W(5) start at 0, 130 chunks"),
    "wrong_extreme": ("W(5) positions", "W(5) start at 0, one chunk"),
    "drop_first_byte_event": ("number positions", "number start at %d, two chunks" % (S.POSITION_N - 151 * 256 - 1)),
    "drop_last_byte_event": ("number positions", "number start at %d, two chunks" % (S.POSITION_N - 151 * 256)),
    "window_restart": ("W(5) positions", "W(5) from 0 end at +257"),
}


@pytest.mark.parametrize("defect", list(FLIPS))
def test_every_defect_flips_a_named_case(defect):
    c = named(*FLIPS[defect])
    assert chunk_route(c) and model(c) == c.want
    assert model(c, defect) != c.want, (defect, c)


def test_the_forward_pass_has_cases_for_its_own_edge_events():
    """The accepting event on the first and on the last byte of a chunk of the FORWARD grid (the two cases above sit on the backward
    grid): an end one byte behind a chunk boundary of the second window, and one on it."""
    first = named("number positions", "number from 0 end at +%d" % (256 + 256 + 1))
    last = named("number positions", "number from 0 end at +%d" % (256 + 256))
    assert model(first, "drop_first_byte_event") != first.want == model(first)
    assert model(last, "drop_last_byte_event") != last.want == model(last)


def test_level_two_reading_the_next_group_flips_the_three_level_case():
    """Backwards over 1024 * 16384 + 1 bytes: 16385 chunks, 129 groups, 2 at level 2.  The match starts in the one-byte chunk walked
    last, whose entry state comes down through level 2: composed from the wrong group, the start is lost."""
    whole, longer = big()
    s, _, _ = tables(whole.pattern)
    t = S.Table(s)
    assert S.directional_run(t, whole.data, True, t.start)[0] == whole.want[0] == 0
    assert S.directional_run(t, whole.data, True, t.start, defect="level2_next_group")[0] != 0
    assert longer.want[0] > S.THREE_LEVELS - 64 and whole.want[1] > S.THREE_LEVELS - 128


def test_level_two_reading_the_next_group_flips_the_forward_three_level_case():
    """Forwards, the sixth window of the 32 MiB + 69 byte string: 16385 chunks, 129 groups, 2 at level 2, entered in the state that
    16 MiB of the match leave (the `c` and 16 MiB - 1 bytes of a/b, a multiple of 5: the residue after the `c` alone).  The match
    ends in the window's last chunk, whose entry state comes down through level 2: composed from the wrong group, the end is lost."""
    whole, longer = S.forward_three_level_cases()
    _, a, _ = tables(whole.pattern)
    t = S.Table(a)
    assert (S.FORWARD_WALKED - 1) % 5 == 0
    entered = int(t.next[t.start, t.col[ord("c")]])
    window = whole.data[S.FORWARD_WALKED:]
    assert S.directional_run(t, window, False, entered, True)[0] == whole.want[1] - S.FORWARD_WALKED
    assert S.directional_run(t, window, False, entered, True, defect="level2_next_group")[0] != whole.want[1] - S.FORWARD_WALKED
    assert longer.want[0] > whole.want[1] and longer.want[1] <= S.FORWARD_THREE_LEVELS
