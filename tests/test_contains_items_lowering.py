"""Contains for explicit items (rrx_contains_extents / rrx_contains_items) on the CPU: the contains table replayed ITEM BY ITEM -
its stride-2 items form (RRX_PROGRAM_CONTAINS_DFA2_ITEMS, kind 18) through Dfa2ItemsReplay, its plain form (kind 16) with '\\n'
stepped through its byte class - against a brute force over the substrings of every item with the oracle's whole-string
acceptance.  '\\n', NUL and bytes >= 0x80 are ordinary text inside an item; nothing rejects."""
import random
import time

import numpy as np

import roaringregex_amd as rr
from contains_cases import EXPLODING, alphabet_for, brute_force, short_line_patterns
from patterns import EMAIL, U2
from program_replay import Dfa2ItemsReplay, DfaReplay
from pyoracle import OracleRegex

# Patterns that take '\n'.  The oracle's dialect cannot spell the byte, so its copy of the pattern has an 'x' in the place of every
# '\n' and sees the items with the same substitution (as test_stripe_wise_items_against_the_oracle does); the alphabet of these
# patterns' items has no 'x' of its own.
NEWLINE_PATTERNS = ["(a|b|\n)*ab(a|\n)*", "k\n+1", "a\nb"]
NEWLINE_ALPHABET = "abck01.d@yz"
MAX_ITEM = 22                                       # the brute force is cubic


def oracle_for(p):
    return OracleRegex(p.replace("\n", "x"))


def as_oracle_sees(p, item):
    return item.replace(b"\n", b"x") if "\n" in p else item


def contains_brute_force(o, item):
    """1 iff some substring of `item`, the empty one included, is accepted as a whole string."""
    n = len(item)
    assert n <= MAX_ITEM
    if o.accepts(b""):
        return 1
    for s in range(n):
        for e in range(s + 1, n + 1):
            if o.accepts(item[s:e]):
                return 1
    return 0


def shortest_accepted(o):
    """A shortest accepted string of the oracle's automaton (breadth first over its states), or None for the empty language."""
    finals = set(o.finals())
    seen, frontier = {o.initial: b""}, [o.initial]
    if o.initial in finals:
        return b""
    while frontier:
        nxt = []
        for s in frontier:
            for c in range(1, 128):
                for t in o.row(s, c):
                    if t not in seen:
                        seen[t] = seen[s] + bytes([c])
                        if t in finals:
                            return seen[t]
                        nxt.append(t)
        frontier = nxt
    return None


def short_items(rng, p, n):
    """Items of at most 22 bytes drawn as contains_cases.short_lines draws lines, with '\\n' in the alphabet: NUL, 0x80, 0xff, a
    two-byte UTF-8 character, empty items - and, one item in nine, a shortest match of the pattern planted at a random place, so
    that patterns a random item hardly ever contains show both verdicts."""
    a = (NEWLINE_ALPHABET if "\n" in p else alphabet_for(p)) + "\n"
    items = ["".join(rng.choice(a) for _ in range(rng.choice([0, 0, 1, 2, 5, 9, 14, 20]))).encode() for _ in range(n)]
    witness = shortest_accepted(oracle_for(p))
    if witness is not None and "\n" in p:
        witness = witness.replace(b"x", b"\n")
    if witness and len(witness) <= MAX_ITEM:
        for i in range(3, n, 9):
            room = MAX_ITEM - len(witness)
            ctx = items[i][:room]
            at = rng.randint(0, len(ctx))
            items[i] = ctx[:at] + witness + ctx[at:]
    items[5] = (b"\x80ab" + items[5])[:MAX_ITEM]
    items[9] = (items[9][:10] + b"\xc3\xa9" + items[10][:10])
    items[13] = (items[13][:8] + b"\x00" + items[14][:8])
    items[20] = b""
    items[21] = b"\n"
    for i in range(31, n, 17):                      # one item in 17 carries a high byte or a NUL somewhere
        it = bytearray(items[i][:20])
        it.insert(rng.randint(0, len(it)), rng.choice([0x00, 0x80, 0xff]))
        items[i] = bytes(it)
    assert all(len(it) <= MAX_ITEM for it in items)
    return items


def want_for(p, items):
    """The brute force per item - and, for the items without '\\n', contains_cases.brute_force on the item as a line: two routes
    through the oracle that must agree."""
    o = oracle_for(p)
    want = np.array([contains_brute_force(o, as_oracle_sees(p, it)) for it in items], dtype=np.uint8)
    flat = [k for k, it in enumerate(items) if b"\n" not in it]
    assert len(flat) >= len(items) // 4
    as_lines = brute_force(p.replace("\n", "x"), b"\n".join(items[k] for k in flat) + b"\n")      # (no '\\n' and no 'x' in these items)
    assert len(as_lines) == len(flat)
    assert (as_lines == want[flat]).all(), (p[:40], "the two oracle routes disagree", items[flat[int(np.nonzero(as_lines != want[flat])[0][0])]])
    return want


def replay_plain(words, items):
    """Kind 16 per item: the start state, every byte - '\\n', NUL and high bytes too - through its class, the verdict of the state."""
    d = DfaReplay(words)
    out = []
    for it in items:
        st = d.start
        for c in it:
            st = int(d.next[st, d.cls[c]])
        out.append(int(d.acc[st]))
    return np.array(out, dtype=np.uint8)


def check(p, items, want, r=None):
    r = r or rr.RRegex(p)
    assert len(want) == len(items)
    got = replay_plain(r.program(rr.PROGRAM_CONTAINS_DFA), items)
    assert got.shape == want.shape                  # (no case is left out)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (p[:40], "kind 16", int(bad[0]), items[bad[0]], int(got[bad[0]]))
    w = r.program(rr.PROGRAM_CONTAINS_DFA2_ITEMS)
    if r.program(rr.PROGRAM_CONTAINS_DFA2) is None:
        assert w is None, (p[:40], "an items form without the stride-2 form")
    if w is not None:
        got2 = np.array(Dfa2ItemsReplay(w).match_items(items), dtype=np.uint8)
        assert got2.shape == want.shape
        bad = np.nonzero(got2 != want)[0]
        assert bad.size == 0, (p[:40], "kind 18", int(bad[0]), items[bad[0]], int(got2[bad[0]]))
    return w is not None


def test_contains_items_programs_against_the_brute_force():
    rng = random.Random(1801)
    pats = short_line_patterns() + ["a*", EMAIL, U2] + NEWLINE_PATTERNS
    with_items_form = 0
    for p in pats:
        r = rr.RRegex(p)
        items = short_items(rng, p, 240)
        want = want_for(p, items)
        if r.accepts_empty:
            assert want.all(), p[:40]
        else:                                       # (against the oracle alone, before any replay)
            assert 0 < int(want.sum()) < len(want), (p[:40], int(want.sum()), len(want))
        with_items_form += check(p, items, want, r)
    assert with_items_form >= len(pats) // 2, with_items_form
    assert rr.RRegex(EMAIL).program(rr.PROGRAM_CONTAINS_DFA2_ITEMS) is not None
    assert rr.RRegex(U2).program(rr.PROGRAM_CONTAINS_DFA2_ITEMS) is None       # (364 states: no stride-2 form, no items table either)


def test_a_match_may_hold_a_newline_and_may_not_straddle_two_items():
    p = "a\nb"
    items = [b"a\nb", b"xa\nby", b"a", b"\nb", b"ab", b"a\n", b"b", b"a\n\nb", b"\n", b"", b"\xffa\nb\x00"]
    want = np.array([1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1], dtype=np.uint8)
    assert check(p, items, want)                    # (kind 18 lays the items end to end: "a\n" + "b" must not be found)
    assert (want_for(p, [it.replace(b"x", b"z").replace(b"y", b"z") for it in items]) == want).all()


def test_nullable_and_empty_language():
    rng = random.Random(1802)
    for p in ("a*", "x?y?z?"):
        items = short_items(rng, p, 60)
        check(p, items, np.ones(len(items), dtype=np.uint8))
    r = rr.RRegex("[]")
    items = short_items(rng, "ab", 60)
    check("[]", items, np.zeros(len(items), dtype=np.uint8), r)


def test_exploding_subset_construction_has_no_items_program_and_does_not_hang():
    r = rr.RRegex(EXPLODING)
    t0 = time.time()
    fwd = r.program(rr.PROGRAM_SEARCH_FWD)              # build_search: the budget the contains build is bounded by
    t_search = time.time() - t0
    r2 = rr.RRegex(EXPLODING)
    t0 = time.time()
    w = r2.program(rr.PROGRAM_CONTAINS_DFA2_ITEMS)
    t_items = time.time() - t0
    assert fwd is None and w is None
    assert r2.contains_states == 0
    assert t_items <= 2 * t_search + 1.0, (t_items, t_search)


def test_forced_byte_stride_engines_have_no_stride2_items_program():
    for p in (EMAIL, "ab+c", "k(1|10|100)"):
        assert rr.RRegex(p).program(rr.PROGRAM_CONTAINS_DFA2_ITEMS) is not None, p
        for e in (rr.ENGINE_DFA, rr.ENGINE_DFA_GLOBAL):
            r = rr.RRegex(p, e)
            assert r.program(rr.PROGRAM_CONTAINS_DFA2_ITEMS) is None, (p, e)
            assert (r.program(rr.PROGRAM_CONTAINS_DFA) == rr.RRegex(p).program(rr.PROGRAM_CONTAINS_DFA)).all()
    # the match engine plays no part: a regex on the NFA lane engine has the same contains programs
    a, b = rr.RRegex(EMAIL, rr.ENGINE_NFA), rr.RRegex(EMAIL)
    assert (a.program(rr.PROGRAM_CONTAINS_DFA2_ITEMS) == b.program(rr.PROGRAM_CONTAINS_DFA2_ITEMS)).all()
