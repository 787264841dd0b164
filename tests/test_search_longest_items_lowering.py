"""Leftmost-longest match per explicit item (rrx_search_longest_extents / rrx_search_longest_items) on the CPU: the starts table
(RRX_PROGRAM_SEARCH_STARTS, kind 19) and the anchored table (RRX_PROGRAM_SEARCH_ANCHORED, kind 20) replayed ITEM BY ITEM exactly as
search_longest_extents_kernel is specified - backward over the whole item to the smallest accepting offset, forward from there to
the last accepting position, stopping in row 0; a nullable pattern runs the forward pass alone from offset 0 - against a brute
force over the substrings of every item with the oracle's whole-string acceptance: the smallest start, then the largest end.
'\\n', NUL and bytes >= 0x80 are ordinary text inside an item.  Also the entries' argument checks, which need no device.

Counts on the shared items (seed 2001, 200 items per pattern, 43 patterns), from the oracle alone: the answer differs from
search_brute_force's (smallest end first) on 577 items of 27 patterns, every time in the END only - random patterns over random
22-byte items hardly ever hold a match that ends before an overlapping match further left does.  The five hand-made START_CASES
supply the items on which the START differs."""
import functools
import random
import re

import numpy as np

import roaringregex_amd as rr
from contains_cases import EXPLODING, short_line_patterns
from program_replay import DfaReplay
from test_contains_items_lowering import MAX_ITEM, NEWLINE_PATTERNS, as_oracle_sees, oracle_for, short_items
from test_search_items_lowering import plain_table_bytes, search_brute_force

NITEMS = 200
SEED = 2001
GLOBAL_AUTO = "x[ab]{12}a[ab]*"                     # its starts table alone passes 64 KiB: AUTO leaves both tables in HBM/L2
# patterns of the long-item tests on the device: Python's greedy search (leftmost start, then - for these two - the longest) names
# the leftmost-longest substring for them; test_greedy_re_names_the_same_substring checks it before anyone relies on it
GREEDY_RE = {"ab+c": rb"ab+c", "a{1,300}": rb"a{1,300}"}
# hand-made items whose leftmost match does not end first: the start differs from search_brute_force's
START_CASES = [("abcd|c", b"abcd"), ("abcd|c", b"zzabcdz"), ("ab+c|b", b"abbc"), ("[0-9]+\\.[0-9]+|\\.", b"12.5"), ("k100|0", b"zk100")]


def longest_brute_force(o, item):
    """(start, end) of the substring of `item` accepted as a whole string with the smallest start, then the largest end; (-1, -1)."""
    n = len(item)
    assert n <= MAX_ITEM
    for s in range(n + 1):
        for e in range(n, s - 1, -1):
            if o.accepts(item[s:e]):
                return s, e
    return -1, -1


def want_for(p, items):
    """int32 [n, 2]: the brute force per item (patterns that take '\\n': through the substitution of test_contains_items_lowering)."""
    o = oracle_for(p)
    return np.array([longest_brute_force(o, as_oracle_sees(p, it)) for it in items], dtype=np.int32).reshape(len(items), 2)


def shortest_for(p, items):
    o = oracle_for(p)
    return np.array([search_brute_force(o, as_oracle_sees(p, it)) for it in items], dtype=np.int32).reshape(len(items), 2)


class SearchLongestReplay:
    """search_longest_extents_kernel per item, in Python ints."""

    def __init__(self, r):
        self.nullable = r.accepts_empty
        s, a = r.program(rr.PROGRAM_SEARCH_STARTS), r.program(rr.PROGRAM_SEARCH_ANCHORED)
        assert s is not None and a is not None
        s, a = DfaReplay(s), DfaReplay(a)
        self.s_cls, self.s_next, self.s_acc, self.s_start = s.cls.tolist(), s.next.tolist(), s.acc.tolist(), s.start
        self.a_cls, self.a_next, self.a_acc, self.a_start = a.cls.tolist(), a.next.tolist(), a.acc.tolist(), a.start
        # what the forward pass' exit relies on: row 0 of the anchored table is dead for good (the packer refuses any other)
        assert not self.a_acc[0] and not any(self.a_next[0])
        self.empty = not any(self.a_acc)            # (the entry: two fills, no table)
        self.hits = self.stopped_early = 0

    def search(self, item):
        if self.empty:
            return -1, -1
        start = 0
        if not self.nullable:
            st, start = self.s_start, None
            for s in range(len(item) - 1, -1, -1):  # the whole item: the starts table has no dead row
                st = self.s_next[st][self.s_cls[item[s]]]
                if self.s_acc[st]:
                    start = s
            if start is None:
                return -1, -1
        self.hits += 1
        st, end = self.a_start, start if self.nullable else None
        for p in range(start, len(item)):
            st = self.a_next[st][self.a_cls[item[p]]]
            if self.a_acc[st]:
                end = p + 1
            if st == 0:
                self.stopped_early += p + 1 < len(item)
                break
        assert end is not None, ("a start without an anchored accept", item, start)
        return start, end

    def search_items(self, items):
        return np.array([self.search(it) for it in items], dtype=np.int32).reshape(len(items), 2)


def check(p, items, want, r=None):
    r = r or rr.RRegex(p)
    rep = SearchLongestReplay(r)
    got = rep.search_items(items)
    assert got.shape == want.shape == (len(items), 2)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (p[:40], int(bad[0]), items[bad[0]], got[bad[0]].tolist(), want[bad[0]].tolist())
    return rep


@functools.lru_cache(maxsize=None)
def reference_set():
    """[(pattern, items, want, shortest)]: the shared patterns and items, the leftmost-longest brute force and search_brute_force's -
    computed once (the device tests share it), never changed."""
    rng = random.Random(SEED)
    out = []
    for p in short_line_patterns() + NEWLINE_PATTERNS:
        items = short_items(rng, p, NITEMS)
        want, short = want_for(p, items), shortest_for(p, items)
        want.setflags(write=False)
        short.setflags(write=False)
        out.append((p, tuple(items), want, short))
    return tuple(out)


def test_search_longest_replay_against_the_brute_force():
    """Measured on these items: 577 items of 27 patterns differ from the smallest-end answer, none of them in the start (the
    module's docstring; test_the_start_differs_from_the_smallest_end_answer has the items that do)."""
    ref = reference_set()
    different = start_different = patterns_different = 0
    for p, items, want, short in ref:               # ---- against the oracle alone, before any replay
        assert any(b"\n" in it for it in items) and any(b"\x00" in it for it in items) and any(b"\x80" in it for it in items)
        assert any(b"\xff" in it for it in items) and any(not it for it in items)
        found = want[:, 1] >= 0
        assert ((want[:, 0] >= 0) == found).all() and (want[:, 0] <= want[:, 1]).all()
        if rr.RRegex(p).accepts_empty:
            assert (want[:, 0] == 0).all(), p[:40]
        else:
            assert 0 < int(found.sum()) < len(items), (p[:40], int(found.sum()))
            assert (want[:, 0] < want[:, 1])[found].all()
        # invariants against the smallest-end answer: the same items match, the start is no larger, the end no smaller
        assert (found == (short[:, 1] >= 0)).all(), p[:40]
        assert (want[found, 0] <= short[found, 0]).all() and (want[found, 1] >= short[found, 1]).all(), p[:40]
        d = (want != short).any(axis=1)
        different += int(d.sum())
        patterns_different += bool(d.any())
        start_different += int((want[:, 0] != short[:, 0]).sum())
    assert different == 577 and patterns_different == 27 and start_different == 0, (different, patterns_different, start_different)
    hits = early = 0
    for p, items, want, _ in ref:
        rep = check(p, items, want)
        hits += rep.hits
        early += rep.stopped_early
    assert hits > 1000 and early > 100, (hits, early)           # (the dead-row exit is exercised, not just present)


def test_the_start_differs_from_the_smallest_end_answer():
    """Hand-made items on which the match that ends first is not the leftmost one."""
    for p, item in START_CASES:
        want, short = want_for(p, [item]), shortest_for(p, [item])
        assert want[0, 0] < short[0, 0] and want[0, 1] >= short[0, 1], (p, item, want.tolist(), short.tolist())
        check(p, [item], want)


def test_named_cases():
    check("[0-9]+", [b"abc 12345 x"], np.array([[4, 9]], dtype=np.int32))
    check("abcd|c", [b"abcd"], np.array([[0, 4]], dtype=np.int32))
    check("ab|b+", [b"abbb"], np.array([[0, 2]], dtype=np.int32))                       # leftmost beats longer
    assert (want_for("[0-9]+", [b"abc 12345 x"]) == [[4, 9]]).all() and (shortest_for("[0-9]+", [b"abc 12345 x"]) == [[4, 5]]).all()
    assert (want_for("abcd|c", [b"abcd"]) == [[0, 4]]).all() and (shortest_for("abcd|c", [b"abcd"]) == [[2, 3]]).all()
    assert (want_for("ab|b+", [b"abbb"]) == [[0, 2]]).all()
    # a match ending exactly at the item's end; one ending at a NUL, one at a 0xff byte
    items = [b"zzab", b"ab", b"abbb", b"zab\x00b", b"abb\xffb", b"\x00ab", b"\xff"]
    want = np.array([[2, 4], [0, 2], [0, 4], [1, 3], [0, 3], [1, 3], [-1, -1]], dtype=np.int32)
    check("ab+", items, want)
    assert (want_for("ab+", items) == want).all()


def test_a_match_may_hold_a_newline_and_stays_inside_its_item():
    p = "a\nb"
    items = [b"a\nb", b"za\nby", b"a", b"\nb", b"ab", b"a\n", b"b", b"a\n\nb", b"\n", b"", b"\xffa\nb\x00", b"a\na\nb"]
    want = np.array([[0, 3], [1, 4], [-1, -1], [-1, -1], [-1, -1], [-1, -1], [-1, -1], [-1, -1], [-1, -1], [-1, -1], [1, 4], [2, 5]], dtype=np.int32)
    check(p, items, want)
    assert (want_for(p, items) == want).all()
    p = "a(\n|b)+"                                               # the longest match runs across newlines
    items = [b"a\nb\n\nbz", b"\na\n", b"a"]
    want = np.array([[0, 6], [1, 3], [-1, -1]], dtype=np.int32)
    check(p, items, want)
    assert (want_for(p, items) == want).all()


def test_nullable_and_empty_language():
    items = [b"aaab", b"baa", b""]
    want = np.array([[0, 3], [0, 0], [0, 0]], dtype=np.int32)
    check("a*", items, want)
    assert (want_for("a*", items) == want).all()
    rng = random.Random(SEED + 1)
    for p in ("a*", "x?y?z?", "(a|b)*c?"):
        items = short_items(rng, p, 60)
        want = want_for(p, items)
        assert (want[:, 0] == 0).all() and (want[:, 1] > 0).any() and (want[:, 1] == 0).any()
        check(p, items, want)
    items = short_items(rng, "ab", 60)
    rep = check("[]", items, np.full((len(items), 2), -1, dtype=np.int32))
    assert rep.empty and not SearchLongestReplay(rr.RRegex("ab")).empty


def test_greedy_re_names_the_same_substring():
    """The long-item device tests take Python's greedy search as their reference beyond 22 bytes: here, on short random items, it is
    the brute force's substring for every pattern they use."""
    rng = random.Random(SEED + 2)
    for p, greedy in GREEDY_RE.items():
        o, c = oracle_for(p), re.compile(greedy)
        n_found = 0
        for _ in range(400):
            item = "".join(rng.choice("aabbc z") for _ in range(rng.randrange(MAX_ITEM + 1))).encode()
            m = c.search(item)
            want = (m.start(), m.end()) if m else (-1, -1)
            assert longest_brute_force(o, item) == want, (p, item)
            n_found += m is not None
        assert n_found > 20, (p, n_found)


def global_auto_items(rng, n):
    items = ["".join(rng.choice("aabbx") for _ in range(rng.choice([0, 3, 13, 14, 15, 20, 22]))).encode() for _ in range(n)]
    return items + [b"x" + b"b" * 12 + b"a", b"x" + b"ab" * 6 + b"ab", b"bx" + b"a" * 13 + b"bbbx", b"x" + b"b" * 11 + b"a", b"x" + b"b" * 13]


def test_tables_beyond_the_lds_budget_and_tables_that_do_not_determinise():
    r = rr.RRegex(GLOBAL_AUTO)
    st, an = r.program(rr.PROGRAM_SEARCH_STARTS), r.program(rr.PROGRAM_SEARCH_ANCHORED)
    assert st is not None and an is not None
    assert plain_table_bytes(st) + plain_table_bytes(an) > 65536, (plain_table_bytes(st), plain_table_bytes(an))
    items = global_auto_items(random.Random(SEED + 3), 120)
    want = want_for(GLOBAL_AUTO, items)
    assert 3 < int((want[:, 1] >= 0).sum()) < len(items)
    check(GLOBAL_AUTO, items, want, r)
    bad = rr.RRegex(EXPLODING)
    assert bad.program(rr.PROGRAM_SEARCH_STARTS) is None and bad.program(rr.PROGRAM_SEARCH_ANCHORED) is None


def test_null_arguments_are_reported_without_a_device():
    r = rr.RRegex("ab+c")
    L = rr._L
    assert L.rrx_search_longest_extents(None, 0, None, None, 0, 0, None, None, None) == 2            # RRX_ERR_ARG
    assert b"null" in L.rrx_last_error()
    buf = (rr.C.c_uint64 * 8)()
    p = rr.C.cast(buf, rr.C.c_void_p)
    assert L.rrx_search_longest_extents(r._h, 0, p, None, 5, 0, p, p, None) == 2                    # no offsets
    assert L.rrx_search_longest_extents(r._h, 0, p, p, 5, 0, None, p, None) == 2                    # no start array
    assert L.rrx_search_longest_extents(r._h, 0, p, p, 5, 0, p, None, None) == 2                    # no end array
    assert L.rrx_search_longest_items(None, None, None, None, None) == 2
    assert L.rrx_search_longest_items(r._h, None, p, p, None) == 2                                  # no items handle
    # a regex whose tables do not determinise is reported before any device call, for an empty batch too
    bad = rr.RRegex(EXPLODING)
    assert L.rrx_search_longest_extents(bad._h, 0, None, None, 0, 0, None, None, None) == 4          # RRX_ERR_UNSUPPORTED
    assert b"determinise" in L.rrx_last_error()
