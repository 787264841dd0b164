"""All matches per explicit item (rrx_search_all_extents* / rrx_search_all_items*) on the CPU: the two plain search tables replayed
ITEM BY ITEM exactly as search_all_extents_kernel is specified - count mode: forward only, the state reset to the start row after
every accepting byte; fill mode: the same forward stream, and after every hit a walk back on the reverse table from the hit end
down to the FLOOR (the end of the previous match), stopping in dead row 0 - against a brute force: test_search_items_lowering's
search_brute_force applied to item[p:] again and again.  Also the entries' argument checks, which need no device."""
import random
import re

import roaringregex_amd as rr
from contains_cases import EXPLODING, short_line_patterns
from program_replay import DfaReplay
from test_contains_items_lowering import MAX_ITEM, NEWLINE_PATTERNS, as_oracle_sees, oracle_for, short_items
from test_search_items_lowering import LAZY_RE, NITEMS, search_brute_force


def all_brute_force(o, item):
    """[(start, end)]: match k = search_brute_force on item[p_k:], p_0 = 0, p_{k+1} = its end, one byte further after an empty match."""
    out, p = [], 0
    while p <= len(item):
        s, e = search_brute_force(o, item[p:])
        if e < 0:
            break
        out.append((p + s, p + e))
        p = p + e if e > s else p + e + 1
    return out


def want_for(p, items):
    """The brute force per item (patterns that take '\\n': through the substitution of test_contains_items_lowering)."""
    o = oracle_for(p)
    return [all_brute_force(o, as_oracle_sees(p, it)) for it in items]


class SearchAllItemsReplay:
    """search_all_extents_kernel per item, in Python ints: count() is its COUNT instantiation, fill() its FILL one."""

    def __init__(self, r, use_floor=True):
        self.nullable = r.accepts_empty
        f, v = DfaReplay(r.program(rr.PROGRAM_SEARCH_FWD)), DfaReplay(r.program(rr.PROGRAM_SEARCH_REV))
        self.f_cls, self.f_next, self.f_acc, self.f_start = f.cls.tolist(), f.next.tolist(), f.acc.tolist(), f.start
        self.r_cls, self.r_next, self.r_acc, self.r_start = v.cls.tolist(), v.next.tolist(), v.acc.tolist(), v.start
        assert not self.r_acc[0] and not any(self.r_next[0])        # the early exit: row 0 of the reverse table is dead for good
        assert self.nullable or not self.f_acc[self.f_start]        # a reset state never accepts: every match has a byte
        self.use_floor = use_floor                                  # (False: what the kernel must NOT do - walk back to the item start)
        self.stopped_early = self.stopped_at_floor = 0

    def count(self, item):
        if self.nullable:                           # (the entry: no table, no text)
            return len(item) + 1
        st, n = self.f_start, 0
        for c in item:
            st = self.f_next[st][self.f_cls[c]]
            if self.f_acc[st]:
                n += 1
                st = self.f_start
        return n

    def fill(self, item):
        if self.nullable:
            return [(k, k) for k in range(len(item) + 1)]
        out, st, floor = [], self.f_start, 0
        for p, c in enumerate(item):
            st = self.f_next[st][self.f_cls[c]]
            if not self.f_acc[st]:
                continue
            st, end = self.f_start, p + 1
            rs, start = self.r_start, None
            for s in range(end - 1, (floor if self.use_floor else 0) - 1, -1):
                rs = self.r_next[rs][self.r_cls[item[s]]]
                if self.r_acc[rs]:
                    start = s
                if rs == 0:
                    self.stopped_early += s > floor
                    break
            else:
                self.stopped_at_floor += floor > 0
            assert start is not None, ("a forward hit without a reverse accept at or above the floor", item, floor, end)
            out.append((start, end))
            floor = end
        return out


def check(p, items, want, r=None):
    rep = SearchAllItemsReplay(r or rr.RRegex(p))
    assert len(items) == len(want)
    for it, w in zip(items, want):
        got = rep.fill(it)
        assert rep.count(it) == len(got), (p[:40], it, rep.count(it), got)
        assert got == w, (p[:40], it, got, w)
    return rep


def test_search_all_items_replay_against_the_brute_force():
    rng = random.Random(1901)
    pats = short_line_patterns() + NEWLINE_PATTERNS
    nullable = multi = total = early = at_floor = 0
    for p in pats:
        r = rr.RRegex(p)
        items = short_items(rng, p, NITEMS)
        want = want_for(p, items)
        if r.accepts_empty:                         # (against the oracle alone, before any replay)
            nullable += 1
            assert all(w == [(k, k) for k in range(len(it) + 1)] for it, w in zip(items, want)), p[:40]
        else:
            multi += any(len(w) >= 2 for w in want)
            total += sum(len(w) for w in want)
            for w in want:                          # non-empty matches, in order, none starting before the end of the one before
                assert all(s < e for s, e in w) and all(w[k][1] <= w[k + 1][0] for k in range(len(w) - 1)), (p[:40], w)
        rep = check(p, items, want, r)
        early += rep.stopped_early
        at_floor += rep.stopped_at_floor
    print("patterns", len(pats), "nullable", nullable, "with an item of two or more matches", multi, "matches", total,
          "walks ended in row 0", early, "at a floor above the item start", at_floor)
    assert multi >= 15, multi
    assert total > 2500, total
    assert early > 100 and at_floor > 0, (early, at_floor)          # (both ends of the walk back are exercised)


def test_a_match_never_starts_before_the_end_of_the_previous_one():
    p = "ab|bab"
    assert want_for(p, [b"abab"]) == [[(0, 2), (2, 4)]]
    check(p, [b"abab", b"bab", b"abbab", b""], [[(0, 2), (2, 4)], [(0, 3)], [(0, 2), (2, 5)], []])
    # the floor is what does it: the same replay walking back to the item start reports the longer substring
    assert SearchAllItemsReplay(rr.RRegex(p), use_floor=False).fill(b"abab") == [(0, 2), (1, 4)]


def test_pinned_cases():
    p = "a*b"
    items = [b"aabaab", b"b", b"bb", b"caabcb", b"aa", b""]
    want = [[(0, 3), (3, 6)], [(0, 1)], [(0, 1), (1, 2)], [(1, 4), (5, 6)], [], []]
    assert want_for(p, items) == want
    check(p, items, want)
    p = "a\nb"
    items = [b"a\nba\nb", b"a\nb", b"za\nb\na\nby", b"a\n", b"a\n\nb", b""]
    want = [[(0, 3), (3, 6)], [(0, 3)], [(1, 4), (5, 8)], [], [], []]
    assert want_for(p, items) == want
    check(p, items, want)


def test_nullable_and_empty_language():
    rng = random.Random(1902)
    for p in ("a*", "x?y?z?"):
        items = short_items(rng, p, 60) + [b""]
        want = [[(k, k) for k in range(len(it) + 1)] for it in items]
        assert want[-1] == [(0, 0)]                 # one match for the empty item
        assert want_for(p, items) == want
        check(p, items, want)
    items = short_items(rng, "ab", 60)
    check("[]", items, [[] for _ in items])
    assert want_for("[]", items[:20]) == [[] for _ in items[:20]]


def lazy_all(p, item):
    return [(m.start(), m.end()) for m in re.finditer(LAZY_RE[p], item)]


def test_lazy_finditer_names_the_same_matches():
    """The long-item and batch-size device tests take re.finditer with the lazy spelling as their reference: here, on short random
    items, it is the brute force's list for every pattern they use."""
    rng = random.Random(1903)
    for p in LAZY_RE:
        o = oracle_for(p)
        n_found = n_multi = 0
        for _ in range(400):
            item = "".join(rng.choice("aabbc z") for _ in range(rng.randrange(MAX_ITEM + 1))).encode()
            want = all_brute_force(o, item)
            assert lazy_all(p, item) == want, (p, item)
            n_found += len(want) >= 1
            n_multi += len(want) >= 2
        assert n_found > 20 and n_multi > 0, (p, n_found, n_multi)


def test_arguments_are_checked_without_a_device():
    r = rr.RRegex("ab+c")
    L, C = rr._L, rr.C
    buf = (C.c_uint64 * 8)()
    p = C.cast(buf, C.c_void_p)
    tot = C.byref(C.c_size_t(0))
    ARG, UNSUPPORTED = 2, 4
    # rrx_search_all_extents_count
    assert L.rrx_search_all_extents_count(None, 0, None, None, 0, 0, None, None) == ARG
    assert b"null" in L.rrx_last_error()
    assert L.rrx_search_all_extents_count(r._h, 0, p, None, 5, 0, p, None) == ARG                   # no offsets
    assert L.rrx_search_all_extents_count(r._h, 0, p, p, 5, 0, None, None) == ARG                   # no counts
    # rrx_search_all_extents_fill
    assert L.rrx_search_all_extents_fill(None, 0, None, None, 0, 0, None, None, None, None) == ARG
    assert L.rrx_search_all_extents_fill(r._h, 0, p, None, 5, 0, p, p, p, None) == ARG              # no offsets
    assert L.rrx_search_all_extents_fill(r._h, 0, p, p, 5, 0, None, p, p, None) == ARG              # no prefix
    assert L.rrx_search_all_extents_fill(r._h, 0, p, p, 5, 0, p, None, p, None) == ARG              # no start array
    assert L.rrx_search_all_extents_fill(r._h, 0, p, p, 5, 0, p, p, None, None) == ARG              # no end array
    # rrx_search_all_extents
    assert L.rrx_search_all_extents(None, 0, None, None, 0, 0, p, None, None, 0, tot, None) == ARG
    assert L.rrx_search_all_extents(r._h, 0, p, p, 5, 0, p, p, p, 9, None, None) == ARG             # no total
    assert L.rrx_search_all_extents(r._h, 0, p, p, 5, 0, None, p, p, 9, tot, None) == ARG           # no prefix
    assert L.rrx_search_all_extents(r._h, 0, None, None, 0, 0, None, None, None, 0, tot, None) == ARG      # ... for an empty batch too
    assert L.rrx_search_all_extents(r._h, 0, p, None, 5, 0, p, p, p, 9, tot, None) == ARG           # no offsets
    assert L.rrx_search_all_extents(r._h, 0, p, p, 5, 0, p, None, p, 9, tot, None) == ARG           # cap > 0 and no start array
    assert L.rrx_search_all_extents(r._h, 0, p, p, 5, 0, p, p, None, 9, tot, None) == ARG           # cap > 0 and no end array
    # the items forms
    assert L.rrx_search_all_items_count(None, None, None, None) == ARG
    assert L.rrx_search_all_items_count(r._h, None, p, None) == ARG                                 # no items handle
    assert L.rrx_search_all_items_fill(None, None, None, None, None, None) == ARG
    assert L.rrx_search_all_items_fill(r._h, None, p, p, p, None) == ARG
    assert L.rrx_search_all_items(None, None, None, None, None, 0, tot, None) == ARG
    assert L.rrx_search_all_items(r._h, None, p, p, p, 9, tot, None) == ARG
    assert b"null" in L.rrx_last_error()
    # a regex without search tables is reported before any device call, for an empty batch too
    bad = rr.RRegex(EXPLODING)
    assert L.rrx_search_all_extents_count(bad._h, 0, None, None, 0, 0, None, None) == UNSUPPORTED
    assert b"determinise" in L.rrx_last_error()
    assert L.rrx_search_all_extents_fill(bad._h, 0, None, None, 0, 0, None, None, None, None) == UNSUPPORTED
    assert L.rrx_search_all_extents(bad._h, 0, None, None, 0, 0, p, None, None, 0, tot, None) == UNSUPPORTED
    assert b"determinise" in L.rrx_last_error()
