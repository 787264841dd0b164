"""All leftmost-longest matches per explicit item (rrx_search_all_longest_extents* / rrx_search_all_longest_items*) on the CPU: the
starts table (kind 19) and the anchored table (kind 20) replayed BATCH BY BATCH as search_all_longest_extents_kernel is specified -
COUNT: backward over the whole item on kind 19, the mark bits of 32 consecutive offsets gathered in a register and stored as the
walk crosses a mark-word boundary downwards and once more at the item's first byte, into ONE flat marks array of the whole batch
(word ((g - base) >> 5) + i, bit (g - base) & 31); then forward: the lane's own words, the bits below p masked off, the first set
bit, kind 20 from there with the dead-row exit before every byte; FILL: the forward phase alone on the marks COUNT left - against a
brute force: test_search_longest_items_lowering's longest_brute_force applied to item[p:] again and again.  Also the entries'
argument checks, which need no device.

Counts on the shared items (test_search_longest_items_lowering.reference_set: seed 2001, 200 items per pattern, 43 patterns), from
the oracle alone: 10729 matches; 1115 items with two or more matches, across 19 patterns; 6 patterns accept the empty string; the
longest match list of one item has 22 entries."""
import functools
import random
import re

import numpy as np

import roaringregex_amd as rr
from contains_cases import EXPLODING
from program_replay import DfaReplay
from test_contains_items_lowering import MAX_ITEM, as_oracle_sees, oracle_for, short_items
from test_search_all_items_lowering import all_brute_force as lazy_all_brute_force
from test_search_longest_items_lowering import GLOBAL_AUTO, SEED, START_CASES, global_auto_items, longest_brute_force, reference_set
from test_search_longest_items_lowering import want_for as first_want_for

POISON = 0x5A5A5A5A
marks_words = rr._L.rrx_search_all_longest_marks_words          # (host only, pure; a library without the entries has no use for this module)
# patterns of the long-item tests on the device, written so that Python's greedy finditer names the leftmost-longest list;
# test_finditer_names_the_same_list checks it before anyone relies on it
GREEDY_ALL_RE = {"ab+c": rb"ab+c", "a{1,300}": rb"a{1,300}", "[0-9]+": rb"[0-9]+"}


def all_longest_brute_force(o, item):
    """[(start, end)]: match k = longest_brute_force on item[p_k:], p_0 = 0, p_{k+1} = its end, one byte further after an empty match."""
    out, p = [], 0
    while p <= len(item):
        s, e = longest_brute_force(o, item[p:])
        if e < 0:
            break
        out.append((p + s, p + e))
        p = p + e if e > s else p + e + 1
    return out


def want_for(p, items):
    """The brute force per item (patterns that take '\\n': through the substitution of test_contains_items_lowering)."""
    o = oracle_for(p)
    return [all_longest_brute_force(o, as_oracle_sees(p, it)) for it in items]


@functools.lru_cache(maxsize=None)
def reference_all():
    """[(pattern, items, want)]: reference_set()'s patterns and items with the iterated brute force - computed once (the device tests
    share it), never changed."""
    return tuple((p, items, tuple(tuple(w) for w in want_for(p, items))) for p, items, _, _ in reference_set())


def pack(items, trim, lead=0, seed=0):
    """items -> (text, offsets): every item followed by `trim` separator bytes of any value, `lead` bytes in front of the first; the
    text ends with the last item's separators."""
    rng = random.Random(seed)
    seps = b"ab\n;\x00\xffc"
    parts, offs, at = [b"q" * lead], [lead], lead
    for it in items:
        parts.append(it + bytes(rng.choice(seps) for _ in range(trim)))
        at += len(it) + trim
        offs.append(at)
    return np.frombuffer(b"".join(parts), dtype=np.uint8).copy(), np.array(offs, dtype=np.int64)


class SearchAllLongestReplay:
    """search_all_longest_extents_kernel on a batch, in Python ints: count() is its COUNT instantiation, fill() its FILL one; both
    work on the batch's flat marks array, as the kernel does."""

    def __init__(self, r):
        self.nullable = r.accepts_empty
        s, a = r.program(rr.PROGRAM_SEARCH_STARTS), r.program(rr.PROGRAM_SEARCH_ANCHORED)
        assert s is not None and a is not None
        s, a = DfaReplay(s), DfaReplay(a)
        self.s_cls, self.s_next, self.s_acc, self.s_start = s.cls.tolist(), s.next.tolist(), s.acc.tolist(), s.start
        self.a_cls, self.a_next, self.a_acc, self.a_start = a.cls.tolist(), a.next.tolist(), a.acc.tolist(), a.start
        assert not self.a_acc[0] and not any(self.a_next[0])        # the forward exit: row 0 of the anchored table is dead for good
        self.empty = not any(self.a_acc)                            # (the entry: the counts are a fill, no table)
        self.walks = self.stopped_early = self.words_skipped = 0

    @staticmethod
    def span(offs, i, trim):
        b, e = int(offs[i]), int(offs[i + 1])
        return b, (e - trim if e - b >= trim else b)

    def _forward(self, text, offs, i, trim, marks):
        """The forward phase of item i -> [(start, end)] relative to the item."""
        base = int(offs[0])
        b, e = self.span(offs, i, trim)
        out, p = [], b
        while True:
            if self.nullable:
                if p > e:
                    break
                s = p
            else:
                s = None
                while p < e:
                    bit = (p - base) & 31
                    m = marks[((p - base) >> 5) + i] & (0xffffffff << bit) & 0xffffffff
                    if m:
                        s = p - bit + ((m & -m).bit_length() - 1)
                        break
                    p = p - bit + 32
                    self.words_skipped += 1
                if s is None:
                    break
                assert s < e, ("a mark behind the item's end", i, s, e)
            st, end, r = self.a_start, s, s
            self.walks += 1
            while r < e:                                            # (the exit is tested before every byte)
                if st == 0:
                    self.stopped_early += 1
                    break
                st = self.a_next[st][self.a_cls[text[r]]]
                r += 1
                if self.a_acc[st]:
                    end = r
            assert self.nullable or end > s, ("a mark without an anchored accept", i, s)
            out.append((s - b, end - b))
            p = end if end > s else s + 1
        return out

    def count(self, text, offs, trim, marks, owner):
        """COUNT on the whole batch: the marks into `marks` (owner[w] = the item that stored word w), -> the counts."""
        n = len(offs) - 1
        if self.empty:
            return [0] * n
        text = text.tolist() if hasattr(text, "tolist") else list(text)
        base = int(offs[0])
        counts = []
        for i in range(n):
            b, e = self.span(offs, i, trim)
            if not self.nullable:
                def put(w, v):
                    assert owner[w] is None, ("word stored twice", w, owner[w], i)
                    owner[w] = i
                    marks[w] = v
                st, acc = self.s_start, 0
                for at in range(e - 1, b - 1, -1):                  # the whole item: the starts table has no dead row
                    st = self.s_next[st][self.s_cls[text[at]]]
                    bit = (at - base) & 31
                    if self.s_acc[st]:
                        acc |= 1 << bit
                    if bit == 0:                                    # crossing a word boundary downwards
                        put(((at - base) >> 5) + i, acc)
                        acc = 0
                if e > b and (b - base) & 31:                       # once more at the item's first byte
                    put(((b - base) >> 5) + i, acc)
            counts.append(len(self._forward(text, offs, i, trim, marks)))
        return counts

    def fill(self, text, offs, trim, marks):
        """FILL on the whole batch, on the marks count() left -> the match list per item."""
        n = len(offs) - 1
        if self.empty:
            return [[] for _ in range(n)]
        text = text.tolist() if hasattr(text, "tolist") else list(text)
        return [self._forward(text, offs, i, trim, marks) for i in range(n)]

    def run(self, items, trim=0, lead=0):
        """One batch through COUNT and FILL with the layout's three properties asserted -> the match list per item."""
        text, offs = pack(items, trim, lead, seed=len(items))
        n, base = len(items), int(offs[0])
        extent = int(offs[-1]) - base
        words = marks_words(extent, n)
        marks, owner = [POISON] * (words + 64), [None] * (words + 64)
        counts = self.count(text, offs, trim, marks, owner)         # (asserts: no word stored by two items)
        written = [w for w, o in enumerate(owner) if o is not None]
        assert not written or max(written) < words, (max(written), words)
        expected = set()                                            # every word of every item's range, all-zero words included
        for i in range(n):
            b, e = self.span(offs, i, trim)
            if e > b and not self.nullable and not self.empty:
                expected |= set(range(((b - base) >> 5) + i, ((e - 1 - base) >> 5) + i + 1))
        assert set(written) == expected
        assert all(marks[w] == POISON for w in range(len(marks)) if w not in expected), "a word outside the items' ranges was touched"
        got = self.fill(text, offs, trim, marks)
        assert counts == [len(g) for g in got]
        return got


def check(p, items, want, r=None, trim=0, lead=0):
    rep = SearchAllLongestReplay(r or rr.RRegex(p))
    got = rep.run(list(items), trim, lead)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == list(w), (p[:40], k, items[k], g, list(w))
    return rep


def test_replay_against_the_iterated_brute_force():
    ref = reference_all()
    # ---- against the oracle alone, before any replay
    total = multi_items = 0
    multi_patterns, nullable, longest = set(), set(), 0
    for p, items, want in ref:
        if rr.RRegex(p).accepts_empty:
            nullable.add(p)
        total += sum(len(w) for w in want)
        m = sum(len(w) >= 2 for w in want)
        multi_items += m
        if m:
            multi_patterns.add(p)
        longest = max(longest, max(len(w) for w in want))
        for it, w in zip(items, want):                              # in order, none starting before the end of the one before
            assert all(0 <= s <= e <= len(it) for s, e in w)
            assert all(w[k][1] <= w[k + 1][0] and w[k] != w[k + 1] for k in range(len(w) - 1)), (p[:40], it, w)
            assert p in nullable or all(s < e for s, e in w)
    print("patterns", len(ref), "matches", total, "items with two or more", multi_items, "in patterns", len(multi_patterns), "nullable",
          len(nullable), "longest list", longest)
    assert len(ref) == 43 and all(len(items) == 200 for _, items, _ in ref)
    assert (total, multi_items, len(multi_patterns), len(nullable), longest) == (10729, 1115, 19, 6, 22)
    # ---- the replay: one flat marks array per batch, base != 0, trim 0 and 1, empty items in between
    walks = early = skipped = 0
    for p, items, want in ref:
        assert any(not it for it in items[1:-1])
        for trim, lead in ((0, 5), (1, 37)):
            rep = check(p, items, want, trim=trim, lead=lead)
            walks += rep.walks
            early += rep.stopped_early
            skipped += rep.words_skipped
    assert walks == 4 * total and early > 1000 and skipped > 100, (walks, early, skipped)      # (COUNT and FILL walk, at both trims; both exits are exercised)


def test_named_cases():
    for p, item, want in (("abcd|c", b"cabcdc", [(0, 1), (1, 5), (5, 6)]), ("ab|b+", b"abbbab", [(0, 2), (2, 4), (4, 6)]),
                          ("[0-9]+", b"a1 22 333", [(1, 2), (3, 5), (6, 9)])):
        assert want_for(p, [item]) == [want], (p, item)
        check(p, [item], [want])
        check(p, [b"", item, b"", item], [[], want, [], want], trim=1, lead=31)
    for p, item in START_CASES:                                     # one match each, the first-match answer
        first = first_want_for(p, [item])
        want = want_for(p, [item])
        assert len(want[0]) == 1 and want[0][0] == tuple(first[0].tolist()), (p, item, want)
        check(p, [item], want)
    # the rule is not rrx_search_all_extents': six one-digit matches there
    assert lazy_all_brute_force(oracle_for("[0-9]+"), b"a1 22 333") == [(1, 2), (3, 4), (4, 5), (6, 7), (7, 8), (8, 9)]


def test_marks_straddle_word_boundaries():
    """Matches at the first and the last bit of a mark word and across one; items that end on, before and behind a boundary."""
    p = "ab+c"
    for lead in (0, 1, 29, 32):
        items = [b"z" * k + b"abc" + b"z" * t for k in (0, 1, 28, 29, 30, 31, 32, 33, 61, 62, 63, 64) for t in (0, 1, 3)]
        items += [b"abc" * 30, b"", b"z" * 64, b"z" * 31 + b"abbc" + b"z" * 29 + b"abc"]
        want = [[(m.start(), m.end()) for m in re.finditer(rb"ab+c", it)] for it in items]
        check(p, items, want, trim=0, lead=lead)
        check(p, items, want, trim=1, lead=lead)


def test_nullable_and_empty_language():
    assert want_for("a*", [b"baab"]) == [[(0, 0), (1, 3), (3, 3), (4, 4)]]
    assert [(m.start(), m.end()) for m in re.finditer(rb"a*", b"baab")] == [(0, 0), (1, 3), (3, 3), (4, 4)]      # Python >= 3.7
    check("a*", [b"baab", b"", b"aa"], [[(0, 0), (1, 3), (3, 3), (4, 4)], [(0, 0)], [(0, 2), (2, 2)]])
    rng = random.Random(SEED + 11)
    for p in ("a*", "x?y?z?", "(a|b)*c?"):
        items = short_items(rng, p, 60) + [b""]
        want = want_for(p, items)
        assert want[-1] == [(0, 0)]                                 # one match for the empty item
        assert any(s < e for w in want for s, e in w) and any(s == e for w in want for s, e in w)
        for trim, lead in ((0, 0), (1, 3)):
            check(p, items, want, trim=trim, lead=lead)
    items = short_items(rng, "ab", 60)
    rep = check("[]", items, [[] for _ in items], lead=2)
    assert rep.empty and not SearchAllLongestReplay(rr.RRegex("ab")).empty
    assert want_for("[]", items[:20]) == [[] for _ in items[:20]]


def test_the_first_match_is_the_leftmost_longest_first_match():
    for (p, items, want), (p2, items2, first, _) in zip(reference_all(), reference_set()):
        assert p == p2 and items == items2
        for k, w in enumerate(want):
            assert (w[0] if w else (-1, -1)) == tuple(first[k].tolist()), (p[:40], items[k])


def test_no_more_matches_than_taken_earliest_end_first():
    """Matches taken earliest-end-first are a maximum set of disjoint matches: the leftmost-longest list is never longer."""
    fewer = 0
    for p, items, want in reference_all():
        if rr.RRegex(p).accepts_empty:
            continue
        o = oracle_for(p)
        for it, w in zip(items, want):
            lazy = lazy_all_brute_force(o, as_oracle_sees(p, it))
            assert len(w) <= len(lazy), (p[:40], it, w, lazy)
            fewer += len(w) < len(lazy)
    assert fewer > 100, fewer


def test_tables_beyond_the_lds_budget():
    r = rr.RRegex(GLOBAL_AUTO)
    items = global_auto_items(random.Random(SEED + 12), 120)
    want = want_for(GLOBAL_AUTO, items)
    # two matches in one item are beyond the brute force's 22 bytes: Python's greedy search names the longest here ([ab]* takes all)
    long_items = [items[-5] + b"b" + items[-4], items[-3] + items[-5], b"x" + items[-5] + b"xx" + items[-4] + b"x"]
    greedy = re.compile(rb"x[ab]{12}a[ab]*")
    assert all([(m.start(), m.end()) for m in greedy.finditer(it)] == w for it, w in zip(items, want))
    items += long_items
    want += [[(m.start(), m.end()) for m in greedy.finditer(it)] for it in long_items]
    assert 3 < sum(bool(w) for w in want) < len(items) and any(len(w) >= 2 for w in want)
    check(GLOBAL_AUTO, items, want, r, trim=1, lead=7)


def finditer_all(p, item):
    return [(m.start(), m.end()) for m in re.finditer(GREEDY_ALL_RE[p], item)]


def test_finditer_names_the_same_list():
    """The long-item device tests take re.finditer as their reference beyond 22 bytes: here, on short random items, it is the brute
    force's list for every pattern they use."""
    rng = random.Random(SEED + 13)
    for p in GREEDY_ALL_RE:
        o = oracle_for(p)
        alphabet = "01 29a" if p == "[0-9]+" else "aabbc z"
        n_found = n_multi = 0
        for _ in range(400):
            item = "".join(rng.choice(alphabet) for _ in range(rng.randrange(MAX_ITEM + 1))).encode()
            want = all_longest_brute_force(o, item)
            assert finditer_all(p, item) == want, (p, item)
            n_found += len(want) >= 1
            n_multi += len(want) >= 2
        assert n_found > 20 and n_multi > 0, (p, n_found, n_multi)


def test_marks_words():
    f = marks_words
    assert f(0, 0) == 1 and f(0, 5) == 6 and f(31, 1) == 2 and f(32, 1) == 3 and f(1000, 10) == 42
    assert f(1 << 40, 1 << 20) == (1 << 35) + (1 << 20) + 1
    # the largest word any item of a batch can own lies below it: item n - 1 ending at the extent's last byte
    for extent, n in ((1, 1), (31, 1), (32, 1), (33, 2), (4096, 64), (4097, 3)):
        assert ((extent - 1) >> 5) + n - 1 < f(extent, n)


def test_arguments_are_checked_without_a_device():
    r = rr.RRegex("ab+c")
    L, C = rr._L, rr.C
    buf = (C.c_uint64 * 8)()
    p = C.cast(buf, C.c_void_p)
    tot = C.byref(C.c_size_t(0))
    ARG, UNSUPPORTED = 2, 4
    # rrx_search_all_longest_extents_count(re, device, bytes, off, nitems, trim, marks, marks_words, count, stream)
    assert L.rrx_search_all_longest_extents_count(None, 0, None, None, 0, 0, None, 0, None, None) == ARG
    assert b"null" in L.rrx_last_error()
    assert L.rrx_search_all_longest_extents_count(r._h, 0, p, None, 5, 0, p, 6, p, None) == ARG          # no offsets
    assert L.rrx_search_all_longest_extents_count(r._h, 0, p, p, 5, 0, None, 6, p, None) == ARG          # no marks
    assert L.rrx_search_all_longest_extents_count(r._h, 0, p, p, 5, 0, p, 6, None, None) == ARG          # no counts
    assert L.rrx_search_all_longest_extents_count(r._h, 0, p, p, 5, 0, p, 5, p, None) == ARG             # marks_words below nitems + 1
    assert b"marks_words" in L.rrx_last_error()
    # rrx_search_all_longest_extents_fill(re, device, bytes, off, nitems, trim, marks, marks_words, first, start, end, stream)
    assert L.rrx_search_all_longest_extents_fill(None, 0, None, None, 0, 0, None, 0, None, None, None, None) == ARG
    assert L.rrx_search_all_longest_extents_fill(r._h, 0, p, None, 5, 0, p, 6, p, p, p, None) == ARG     # no offsets
    assert L.rrx_search_all_longest_extents_fill(r._h, 0, p, p, 5, 0, None, 6, p, p, p, None) == ARG     # no marks
    assert L.rrx_search_all_longest_extents_fill(r._h, 0, p, p, 5, 0, p, 5, p, p, p, None) == ARG        # marks_words below nitems + 1
    assert L.rrx_search_all_longest_extents_fill(r._h, 0, p, p, 5, 0, p, 6, None, p, p, None) == ARG     # no prefix
    assert L.rrx_search_all_longest_extents_fill(r._h, 0, p, p, 5, 0, p, 6, p, None, p, None) == ARG     # no start array
    assert L.rrx_search_all_longest_extents_fill(r._h, 0, p, p, 5, 0, p, 6, p, p, None, None) == ARG     # no end array
    # rrx_search_all_longest_extents(re, device, bytes, off, nitems, trim, first, start, end, cap, total, stream)
    assert L.rrx_search_all_longest_extents(None, 0, None, None, 0, 0, p, None, None, 0, tot, None) == ARG
    assert L.rrx_search_all_longest_extents(r._h, 0, p, p, 5, 0, p, p, p, 9, None, None) == ARG          # no total
    assert L.rrx_search_all_longest_extents(r._h, 0, p, p, 5, 0, None, p, p, 9, tot, None) == ARG        # no prefix
    assert L.rrx_search_all_longest_extents(r._h, 0, None, None, 0, 0, None, None, None, 0, tot, None) == ARG      # ... for an empty batch too
    assert L.rrx_search_all_longest_extents(r._h, 0, p, None, 5, 0, p, p, p, 9, tot, None) == ARG        # no offsets
    assert L.rrx_search_all_longest_extents(r._h, 0, p, p, 5, 0, p, None, p, 9, tot, None) == ARG        # cap > 0 and no start array
    assert L.rrx_search_all_longest_extents(r._h, 0, p, p, 5, 0, p, p, None, 9, tot, None) == ARG        # cap > 0 and no end array
    # the items forms
    assert L.rrx_search_all_longest_items_count(None, None, None, 0, None, None) == ARG
    assert L.rrx_search_all_longest_items_count(r._h, None, p, 6, p, None) == ARG                        # no items handle
    assert L.rrx_search_all_longest_items_fill(None, None, None, 0, None, None, None, None) == ARG
    assert L.rrx_search_all_longest_items_fill(r._h, None, p, 6, p, p, p, None) == ARG
    assert L.rrx_search_all_longest_items(None, None, None, None, None, 0, tot, None) == ARG
    assert L.rrx_search_all_longest_items(r._h, None, p, p, p, 9, tot, None) == ARG
    assert b"null" in L.rrx_last_error()


def test_a_regex_without_tables_is_reported_for_an_empty_batch_without_a_device():
    L, C = rr._L, rr.C
    p = C.cast((C.c_uint64 * 8)(), C.c_void_p)
    tot = C.byref(C.c_size_t(0))
    bad = rr.RRegex(EXPLODING)
    assert bad.program(rr.PROGRAM_SEARCH_STARTS) is None and bad.program(rr.PROGRAM_SEARCH_ANCHORED) is None
    assert L.rrx_search_all_longest_extents_count(bad._h, 0, None, None, 0, 0, None, 0, None, None) == 4       # RRX_ERR_UNSUPPORTED
    assert b"determinise" in L.rrx_last_error()
    assert L.rrx_search_all_longest_extents_fill(bad._h, 0, None, None, 0, 0, None, 0, None, None, None, None) == 4
    assert L.rrx_search_all_longest_extents(bad._h, 0, None, None, 0, 0, p, None, None, 0, tot, None) == 4
    assert b"determinise" in L.rrx_last_error()
