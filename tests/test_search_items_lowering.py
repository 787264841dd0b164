"""First match per explicit item (rrx_search_extents / rrx_search_items) on the CPU: the two plain search tables
(RRX_PROGRAM_SEARCH_FWD, kind 6, and RRX_PROGRAM_SEARCH_REV, kind 7) replayed ITEM BY ITEM exactly as search_extents_kernel is
specified - forward to the first accepting position, backward from there to the last accepting one, stopping in row 0 - against a
brute force over the substrings of every item with the oracle's whole-string acceptance: the smallest end, then the smallest
start.  '\\n', NUL and bytes >= 0x80 are ordinary text inside an item.  Also the entries' argument checks, which need no device."""
import random
import re

import numpy as np

import roaringregex_amd as rr
from contains_cases import EXPLODING, short_line_patterns
from program_replay import DfaReplay
from table_edge_cases import plain_table_bytes
from test_contains_items_lowering import MAX_ITEM, NEWLINE_PATTERNS, as_oracle_sees, oracle_for, short_items

NITEMS = 200
GLOBAL_AUTO = "[ab]*a[ab]{12}x"                     # its two plain tables together pass 64 KiB: AUTO leaves them in HBM/L2
# patterns of the long-item tests on the device: Python's lazy search (leftmost start, then shortest) and "smallest end, then
# smallest start" name the same substring for them - test_lazy_re_names_the_same_substring checks it before anyone relies on it
LAZY_RE = {"ab+c": rb"ab+?c", "a{1,300}": rb"a{1,300}?"}


def search_brute_force(o, item):
    """(start, end) of the substring of `item` accepted as a whole string with the smallest end, then the smallest start; (-1, -1)."""
    n = len(item)
    assert n <= MAX_ITEM
    if o.accepts(b""):
        return 0, 0
    for e in range(1, n + 1):
        for s in range(e):
            if o.accepts(item[s:e]):
                return s, e
    return -1, -1


def want_for(p, items):
    """int32 [n, 2]: the brute force per item (patterns that take '\\n': through the substitution of test_contains_items_lowering)."""
    o = oracle_for(p)
    return np.array([search_brute_force(o, as_oracle_sees(p, it)) for it in items], dtype=np.int32).reshape(len(items), 2)


class SearchItemsReplay:
    """search_extents_kernel per item, in Python ints."""

    def __init__(self, r):
        self.nullable = r.accepts_empty
        f, v = DfaReplay(r.program(rr.PROGRAM_SEARCH_FWD)), DfaReplay(r.program(rr.PROGRAM_SEARCH_REV))
        self.f_cls, self.f_next, self.f_acc, self.f_start = f.cls.tolist(), f.next.tolist(), f.acc.tolist(), f.start
        self.r_cls, self.r_next, self.r_acc, self.r_start = v.cls.tolist(), v.next.tolist(), v.acc.tolist(), v.start
        # what the kernel's early exit relies on: row 0 of the reverse table is dead for good
        assert not self.r_acc[0] and not any(self.r_next[0])
        self.hits = self.stopped_early = 0

    def search(self, item):
        if self.nullable:                           # (the entry: two fills, no table)
            return 0, 0
        st, end = self.f_start, -1
        for p, c in enumerate(item):
            st = self.f_next[st][self.f_cls[c]]
            if self.f_acc[st]:
                end = p + 1
                break
        if end < 0:
            return -1, -1
        self.hits += 1
        st, start = self.r_start, None
        for s in range(end - 1, -1, -1):
            st = self.r_next[st][self.r_cls[item[s]]]
            if self.r_acc[st]:
                start = s
            if st == 0:
                self.stopped_early += s > 0
                break
        assert start is not None, ("a forward hit without a reverse accept", item, end)
        return start, end

    def search_items(self, items):
        return np.array([self.search(it) for it in items], dtype=np.int32).reshape(len(items), 2)


def check(p, items, want, r=None):
    r = r or rr.RRegex(p)
    rep = SearchItemsReplay(r)
    got = rep.search_items(items)
    assert got.shape == want.shape == (len(items), 2)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (p[:40], int(bad[0]), items[bad[0]], got[bad[0]].tolist(), want[bad[0]].tolist())
    return rep


def test_search_items_replay_against_the_brute_force():
    rng = random.Random(1901)
    hits = early = 0
    for p in short_line_patterns() + NEWLINE_PATTERNS:
        r = rr.RRegex(p)
        items = short_items(rng, p, NITEMS)
        assert any(b"\n" in it for it in items) and any(b"\x00" in it for it in items) and any(b"\x80" in it for it in items)
        assert any(b"\xff" in it for it in items) and any(not it for it in items)
        want = want_for(p, items)
        if r.accepts_empty:
            assert (want == 0).all(), p[:40]
        else:                                       # (against the oracle alone, before any replay: both verdicts occur)
            found = int((want[:, 1] >= 0).sum())
            assert 0 < found < len(items), (p[:40], found)
            assert ((want[:, 0] >= 0) == (want[:, 1] >= 0)).all() and (want[:, 0] < want[:, 1])[want[:, 1] >= 0].all()
        rep = check(p, items, want, r)
        hits += rep.hits
        early += rep.stopped_early
    assert hits > 1000 and early > 100, (hits, early)           # (the dead-row exit is exercised, not just present)


def test_a_match_may_hold_a_newline_and_stays_inside_its_item():
    p = "a\nb"
    items = [b"a\nb", b"za\nby", b"a", b"\nb", b"ab", b"a\n", b"b", b"a\n\nb", b"\n", b"", b"\xffa\nb\x00", b"a\na\nb"]
    want = np.array([[0, 3], [1, 4], [-1, -1], [-1, -1], [-1, -1], [-1, -1], [-1, -1], [-1, -1], [-1, -1], [-1, -1], [1, 4], [2, 5]], dtype=np.int32)
    check(p, items, want)
    assert (want_for(p, items) == want).all()


def test_smallest_end_then_smallest_start():
    # "bc" ends first in "abcc"; among the substrings that end there, the one from 'a' starts first
    check("abc|bc|abcc", [b"abcc", b"zbcc", b"ab"], np.array([[0, 3], [1, 3], [-1, -1]], dtype=np.int32))
    # the walk back goes on past an accepting position: "aab" accepts from 1 and from 0
    check("a*b", [b"aab", b"caab", b"b"], np.array([[0, 3], [1, 4], [0, 1]], dtype=np.int32))
    assert (want_for("abc|bc|abcc", [b"abcc"]) == [[0, 3]]).all() and (want_for("a*b", [b"caab"]) == [[1, 4]]).all()


def test_nullable_and_empty_language():
    rng = random.Random(1902)
    for p in ("a*", "x?y?z?"):
        items = short_items(rng, p, 60)
        check(p, items, np.zeros((len(items), 2), dtype=np.int32))
        assert (want_for(p, items) == 0).all()
    items = short_items(rng, "ab", 60)
    check("[]", items, np.full((len(items), 2), -1, dtype=np.int32))


def test_lazy_re_names_the_same_substring():
    """The long-item device tests take Python's lazy search as their reference beyond 22 bytes: here, on short random items, it is
    the brute force's substring for every pattern they use."""
    rng = random.Random(1903)
    for p, lazy in LAZY_RE.items():
        o, c = oracle_for(p), re.compile(lazy)
        n_found = 0
        for _ in range(400):
            item = "".join(rng.choice("aabbc z") for _ in range(rng.randrange(MAX_ITEM + 1))).encode()
            m = c.search(item)
            want = (m.start(), m.end()) if m else (-1, -1)
            assert search_brute_force(o, item) == want, (p, item)
            n_found += m is not None
        assert n_found > 20, (p, n_found)


def test_the_plain_tables_are_dumped_whether_or_not_the_stripe_wise_kernel_fits():
    r = rr.RRegex(GLOBAL_AUTO)
    fw, rv = r.program(rr.PROGRAM_SEARCH_FWD), r.program(rr.PROGRAM_SEARCH_REV)
    assert fw is not None and rv is not None
    assert plain_table_bytes(fw) + plain_table_bytes(rv) > 65536, (plain_table_bytes(fw), plain_table_bytes(rv))
    rng = random.Random(1904)
    items = ["".join(rng.choice("abx") for _ in range(rng.choice([0, 3, 13, 14, 15, 20, 22]))).encode() for _ in range(120)]
    items += [b"a" + b"b" * 12 + b"x", b"b" * 7 + b"a" + b"ab" * 6 + b"x", b"a" + b"b" * 11 + b"x"]
    want = want_for(GLOBAL_AUTO, items)
    assert 0 < int((want[:, 1] >= 0).sum()) < len(items)
    check(GLOBAL_AUTO, items, want, r)
    bad = rr.RRegex(EXPLODING)
    assert bad.program(rr.PROGRAM_SEARCH_FWD) is None


def test_null_arguments_are_reported_without_a_device():
    r = rr.RRegex("ab+c")
    L = rr._L
    assert L.rrx_search_extents(None, 0, None, None, 0, 0, None, None, None) == 2                    # RRX_ERR_ARG
    assert b"null" in L.rrx_last_error()
    buf = (rr.C.c_uint64 * 8)()
    p = rr.C.cast(buf, rr.C.c_void_p)
    assert L.rrx_search_extents(r._h, 0, p, None, 5, 0, p, p, None) == 2                            # no offsets
    assert L.rrx_search_extents(r._h, 0, p, p, 5, 0, None, p, None) == 2                            # no start array
    assert L.rrx_search_extents(r._h, 0, p, p, 5, 0, p, None, None) == 2                            # no end array
    assert L.rrx_search_items(None, None, None, None, None) == 2
    assert L.rrx_search_items(r._h, None, p, p, None) == 2                                          # no items handle
    # a regex without search tables is reported before any device call, for an empty batch too
    bad = rr.RRegex(EXPLODING)
    assert L.rrx_search_extents(bad._h, 0, None, None, 0, 0, None, None, None) == 4                  # RRX_ERR_UNSUPPORTED
    assert b"determinise" in L.rrx_last_error()
