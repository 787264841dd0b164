"""regexp_replace with group references (rrx_template_*, rrx_group_spans_list_*, rrx_replace_template_*, rrx_replace_groups_longest_*)
on the CPU: the template parser through rrx_template_segments / _refs and its return codes; the return codes of every new entry for
null and inconsistent arguments, which need no device; longest_split_list_kernel replayed in Python ints AS IT IS SPECIFIED - a lane
per item walking its slots, the two phases of longest_split_kernel per slot on ONE flat marks array - against the brute force of the
group rule of test_group_items_lowering applied to every match of the iterated leftmost-longest list; and both kernels of
kernels_replace_template_items.hip replayed - the one walk over the segments that both passes share, the sizes a lane per item, the
fill a wave per 64 items driven by output bytes with the segment level in locate - against a pure-Python splice and, where
test_group_items_lowering shows that Python's rule is ours, against re.sub."""
import functools
import random
import re

import pytest

import roaringregex_amd as rr
from test_contains_items_lowering import MAX_ITEM
from test_group_items_lowering import NAMED, GroupReplay, group_brute_force, oracles_for
from test_replace_items_lowering import M64, MARGIN, csr_lists, span, splice
from test_search_all_longest_items_lowering import POISON, all_longest_brute_force, marks_words, pack
from test_search_longest_items_lowering import SEED

OK, PATTERN, ARG, UNSUPPORTED = 0, 1, 2, 4
NONE = 0xFFFFFFFF
OUT_POISON = 0x5A
DATE = "([0-9]+)/([0-9]+)/([0-9]+)"
# (pattern, number of top-level groups, alphabet, plants): every group is at the top level and not repeated
CASES = ((DATE, 3, "0199/ x", (b"1/2/3", b"12/31/1999", b"1/2/3/4/5/6", b"9/9/99/9/9")), ("([0-9]+)-([0-9]+)", 2, "019- x", (b"1-0", b"90-11-9")),
         ("x(a*)", 1, "xab", ()), ("(a*)(b*)", 2, "abc", ()), ("(ab|a)(b*)", 2, "abc", ()), ("[ab]+(b*)[ab]+", 1, "abx", ()),
         ("a*(a*)a*", 1, "aab", ()))
# templates as the user writes them; the last one has 32 segments
TEMPLATES = (b"", b"<lit>", rb"\0", rb"\1\1", rb"\2-\1", rb"\1 to \0 and \\ then \2", rb"\3-\1-\2", rb"[\12]", b"".join(b"%c\\1" % (65 + k) for k in range(16)))


def parse_py(repl):
    """The template's segments by the rule of include/rrx.h, written again in Python: bytes for a literal, an int for a reference."""
    out, p = [], 0
    while p < len(repl):
        c = repl[p:p + 1]
        if c == b"\\":
            nxt = repl[p + 1:p + 2]
            assert nxt and (nxt == b"\\" or nxt.isdigit()), (repl, p)
            c, p = (b"\\" if nxt == b"\\" else int(nxt)), p + 1
        if isinstance(c, bytes) and out and isinstance(out[-1], bytes):
            out[-1] += c
        else:
            out.append(c)
        p += 1
    return tuple(out)


def span_group(p, g, item, s, e):
    """The group rule of include/rrx.h for the span [s, e) of `item` - test_group_items_lowering's admissible() for any span; (-1, -1)
    where the span has no split."""
    _, a, b, c = oracles_for(p, g)
    bc = lambda i: [j for j in range(i, e + 1) if b.accepts(item[i:j]) and c.accepts(item[j:e])]
    i_s = [i for i in range(s, e + 1) if a.accepts(item[s:i]) and bc(i)]
    return (max(i_s), max(bc(max(i_s)))) if i_s else (-1, -1)


def expand(segs, item, match, groups):
    """The replacement of one match: groups = {g: (i, j)}; a span (-1, -1) contributes nothing."""
    out = []
    for seg in segs:
        if isinstance(seg, bytes):
            out.append(seg)
        else:
            s, e = match if seg == 0 else groups[seg]
            if s >= 0:
                out.append(item[s:e])
    return b"".join(out)


def splice_template(item, matches, spans, segs):
    """The rule: the item with match k replaced by R_k; spans = {g: [(i, j) per match]}."""
    out, at = [], 0
    for k, (s, e) in enumerate(matches):
        assert at <= s <= e <= len(item)
        out += [item[at:s], expand(segs, item, (s, e), {g: w[k] for g, w in spans.items()})]
        at = e
    out.append(item[at:])
    return b"".join(out)


def items_for(alphabet, plants, rng, n):
    items = ["".join(rng.choice(alphabet) for _ in range(rng.choice([0, 1, 3, 5, 8, 12, 17, MAX_ITEM]))).encode() for _ in range(n)]
    for k in range(2, n, 3):
        if plants:
            plant, at = rng.choice(plants), rng.randint(0, len(items[k]))
            items[k] = (items[k][:at] + plant + items[k][at:])[:MAX_ITEM]
    items[3] = items[n // 2] = b""
    return items


@functools.lru_cache(maxsize=None)
def reference_templates():
    """[(pattern, ngroups, items, lists, {g: [[(i, j) per match] per item]})]: computed once (the device tests share it), never changed."""
    rng = random.Random(SEED + 31)
    out = []
    for p, ngroups, alphabet, plants in CASES:
        items = tuple(items_for(alphabet, plants, rng, 90))
        whole = oracles_for(p, 1)[0]
        lists = tuple(tuple(all_longest_brute_force(whole.o, it)) for it in items)
        spans = {g: tuple(tuple(span_group(p, g, it, s, e) for s, e in w) for it, w in zip(items, lists)) for g in range(1, ngroups + 1)}
        out.append((p, ngroups, items, lists, spans))
    return tuple(out)


def expected_items(items, lists, spans, repl):
    segs = parse_py(repl)
    return [splice_template(it, w, {g: sp[k] for g, sp in spans.items()}, segs) for k, (it, w) in enumerate(zip(items, lists))]


# ------------------------------------------------------------------------------------------------ the template parser
def compile_code(repl):
    h = rr.C.c_void_p()
    rc = rr._L.rrx_template_compile(repl, len(repl), rr.C.byref(h))
    err = rr._L.rrx_last_error()
    assert bool(h.value) == (rc == OK)
    if h.value:
        rr._L.rrx_template_free(h)
    return rc, err


def test_the_parser():
    T = rr.Template
    assert T(b"").segments == () and T(b"").refs == ()
    assert T(b"abc").segments == (b"abc",) and T(b"abc").refs == ()
    assert T(rb"\0").segments == (0,) and T(rb"\0").refs == ()                   # the whole match is no plane
    assert T(rb"\3-\1-\2").segments == (3, b"-", 1, b"-", 2) and T(rb"\3-\1-\2").refs == (1, 2, 3)
    assert T(rb"\12").segments == (1, b"2") and T(rb"\12").refs == (1,)          # one digit
    assert T(rb"a\\b").segments == (b"a\\b",)                                    # \\ is a backslash and merges with its neighbours
    assert T(rb"\\\\").segments == (b"\\\\",) and T(rb"\\1").segments == (b"\\1",)
    assert T(rb"\9x\9\0\9").segments == (9, b"x", 9, 0, 9) and T(rb"\9x\9\0\9").refs == (9,)
    assert T(b"\x00\xff\n").segments == (b"\x00\xff\n",)                         # every byte but the backslash is literal
    assert T("\\2-\\1").segments == (2, b"-", 1)                                 # str: latin-1
    for repl in TEMPLATES:
        assert T(repl).segments == parse_py(repl), repl
        assert T(repl).refs == tuple(sorted({s for s in parse_py(repl) if isinstance(s, int) and s > 0})), repl
    assert len(T(TEMPLATES[-1]).segments) == 32
    # every error with its offset
    for repl, at in ((b"\\", 0), (b"ab\\", 2), (rb"a\x", 1), (rb"\1\2\g<1>", 4), (b"\\\\\\", 2), (rb"\0\ ", 2), (b"x\\\n", 1)):
        rc, err = compile_code(repl)
        assert rc == PATTERN and (b"offset %d " % at) in err, (repl, err)
        with pytest.raises(rr.RRegexError):
            T(repl)
    # 33 segments are one too many; 32 literal bytes between them do not count, they merge
    rc, err = compile_code(TEMPLATES[-1] + b"x")
    assert rc == UNSUPPORTED and b"32" in err
    assert compile_code(b"\\1" * 32)[0] == OK and compile_code(b"\\1" * 33)[0] == UNSUPPORTED and compile_code(b"x" * 1000)[0] == OK
    # the dumps write nothing past cap and return the counts
    t = T(rb"ab\2cd\1")
    refs, lens = (rr.C.c_int * 4)(7, 7, 7, 7), (rr.C.c_uint32 * 4)(7, 7, 7, 7)
    lits = rr.C.create_string_buffer(b"####", 4)
    assert rr._L.rrx_template_segments(t._h, refs, lens, 2, lits, 3) == 4 and list(refs) == [-1, 2, 7, 7] and list(lens) == [2, 0, 7, 7] and lits.raw == b"abc#"
    groups = (rr.C.c_int * 2)(7, 7)
    assert rr._L.rrx_template_refs(t._h, groups, 1) == 2 and list(groups) == [1, 7]
    assert rr._L.rrx_template_refs(None, groups, 2) == 0 and rr._L.rrx_template_segments(None, None, None, 0, None, 0) == 0
    h = rr.C.c_void_p()
    assert rr._L.rrx_template_compile(b"x", 1, None) == ARG and rr._L.rrx_template_compile(None, 1, rr.C.byref(h)) == ARG
    assert rr._L.rrx_template_compile(None, 0, rr.C.byref(h)) == OK                # the empty template needs no bytes
    rr._L.rrx_template_free(h)
    rr._L.rrx_template_free(None)


# ------------------------------------------------------------------------------------------------ the entries' argument checks
def test_arguments_are_checked_without_a_device():
    L, C = rr._L, rr.C
    g = rr.RGroup("a(b+)c", 1)
    bare = rr.RGroup("(b+)", 1)
    p = C.cast((C.c_uint64 * 8)(), C.c_void_p)
    tot = C.byref(C.c_size_t(0))
    # rrx_group_spans_list_extents(grp, device, bytes, off, nitems, trim, first, match_start, match_end, marks, marks_words, group_start, group_end, stream)
    ok = [g._h, 0, p, p, 5, 0, p, p, p, p, 6, p, p, None]
    for k in (0, 3, 6, 7, 8, 9, 11, 12):
        a = list(ok)
        a[k] = None
        assert L.rrx_group_spans_list_extents(*a) == ARG, k
        assert b"null" in L.rrx_last_error()
    a = list(ok)
    a[10] = 5
    assert L.rrx_group_spans_list_extents(*a) == ARG and b"marks_words" in L.rrx_last_error()
    assert L.rrx_group_spans_list_extents(bare._h, 0, p, p, 5, 0, None, p, p, None, 0, p, p, None) == ARG      # marks may be null here, the prefix may not
    assert L.rrx_group_spans_list_extents(g._h, 0, None, None, 0, 0, None, None, None, None, 0, None, None, None) == OK
    assert L.rrx_group_spans_list_items(None, None, None, None, None, None, 0, None, None, None) == ARG
    assert L.rrx_group_spans_list_items(g._h, None, p, p, p, p, 6, p, p, None) == ARG                         # no items handle
    # rrx_replace_template_sizes(device, off, nitems, trim, first, start, end, tpl, ref_start, ref_end, plane_stride, len, pos, stream)
    plain, refs = rr.Template(rb"<\0>"), rr.Template(rb"\2-\1")
    ok = [0, p, 5, 0, p, p, p, refs._h, p, p, 9, p, p, None]
    for k in (1, 4, 5, 6, 7, 8, 9, 11, 12):
        a = list(ok)
        a[k] = None
        assert L.rrx_replace_template_sizes(*a) == ARG, k
        assert b"null" in L.rrx_last_error()
    assert L.rrx_replace_template_sizes(0, None, 0, 0, None, None, None, refs._h, None, None, 0, None, None, None) == OK      # nitems == 0
    assert L.rrx_replace_template_sizes(0, None, 0, 0, None, None, None, None, None, None, 0, None, None, None) == ARG        # ... but a template
    for k in (1, 4, 5, 6, 7, 11, 12):                                            # no reference to a group: the planes may be null, nothing else
        a = [0, p, 5, 0, p, p, p, plain._h, None, None, 0, p, p, None]
        a[k] = None
        assert L.rrx_replace_template_sizes(*a) == ARG, k
    # rrx_replace_template_fill(device, bytes, off, nitems, trim, first, start, end, pos, tpl, ref_start, ref_end, plane_stride, out_off, out, stream)
    ok = [0, p, p, 5, 0, p, p, p, p, refs._h, p, p, 9, p, p, None]
    for k in (2, 5, 6, 7, 8, 9, 10, 11, 13):
        a = list(ok)
        a[k] = None
        assert L.rrx_replace_template_fill(*a) == ARG, k
    assert L.rrx_replace_template_fill(0, None, None, 0, 0, None, None, None, None, refs._h, None, None, 0, None, None, None) == OK
    for k in (2, 5, 6, 7, 8, 9, 13):
        a = [0, p, p, 5, 0, p, p, p, p, plain._h, None, None, 0, p, p, None]
        a[k] = None
        assert L.rrx_replace_template_fill(*a) == ARG, k
    # rrx_replace_groups_longest_extents(groups, ngroups, tpl, device, bytes, off, nitems, trim, out_off, out, cap, total, stream)
    g1, g2, other = rr.RGroup("([0-9]+)-([0-9]+)", 1), rr.RGroup("([0-9]+)-([0-9]+)", 2), rr.RGroup("([0-9]+)_([0-9]+)", 2)
    handles = lambda *gs: (C.c_void_p * len(gs))(*[x._h if x is not None else None for x in gs])
    both = handles(g1, g2)
    ok = [both, 2, refs._h, 0, p, p, 5, 0, p, p, 9, tot, None]
    for k in (0, 2, 5, 8, 9, 11):
        a = list(ok)
        a[k] = None
        assert L.rrx_replace_groups_longest_extents(*a) == ARG, k
        assert b"null" in L.rrx_last_error()
    assert L.rrx_replace_groups_longest_extents(handles(None, None), 2, plain._h, 0, p, p, 5, 0, p, p, 9, tot, None) == ARG
    assert b"no group handle" in L.rrx_last_error()
    assert L.rrx_replace_groups_longest_extents(both, 0, plain._h, 0, p, p, 5, 0, p, p, 9, tot, None) == ARG                # ngroups == 0: no handle either
    assert L.rrx_replace_groups_longest_extents(handles(g1, other), 2, refs._h, 0, p, p, 5, 0, p, p, 9, tot, None) == ARG  # handles of two patterns
    assert b"one pattern" in L.rrx_last_error()
    assert L.rrx_replace_groups_longest_extents(handles(g1, None), 2, refs._h, 0, p, p, 5, 0, p, p, 9, tot, None) == ARG   # \2 without a handle
    assert b"group 2" in L.rrx_last_error()
    assert L.rrx_replace_groups_longest_extents(handles(g1), 1, refs._h, 0, p, p, 5, 0, p, p, 9, tot, None) == ARG         # ... and beyond ngroups
    assert L.rrx_replace_groups_longest_extents(both, 2, refs._h, 0, None, None, 0, 0, None, None, 0, tot, None) == ARG    # no d_out_off, for an empty batch too
    assert L.rrx_replace_groups_longest_items(both, 2, refs._h, None, p, p, 9, tot, None) == ARG                           # no items handle
    assert L.rrx_replace_groups_longest_items(None, 2, refs._h, None, p, p, 9, tot, None) == ARG
    # the Python layer refuses the same
    with pytest.raises(AssertionError):
        rr.replace_groups_longest_extents([], refs, None, None)


# ------------------------------------------------------------------------------------------------ the list-spans kernel
class ListReplay(GroupReplay):
    """longest_split_list_kernel on a batch, in Python ints: a lane per item, its slots in order, per slot the two phases of
    longest_split_kernel (GroupReplay.launch has them for one stretch per item) on the batch's ONE flat marks array."""

    def launch_list(self, text, offs, trim, first, lo_in, hi_in, rev, fwd, marks, nwords, out, on_none):
        """One launch; lo_in / hi_in / out / on_none are indexed by the slot and may be the same lists.  -> {item: the words it
        stored}.  A word may be stored more than once - by consecutive slots of ONE item."""
        r_cls, r_next, r_acc, r_start = self.tables[rev]
        f_cls, f_next, f_acc, f_start = self.tables[fwd]
        base, n = int(offs[0]), len(offs) - 1
        stored = {}
        for i in range(n):
            b, e = self.span(offs, i, trim)
            word_of = lambda g: ((g - base) >> 5) + i
            mine = stored.setdefault(i, set())

            def put(w, v):
                mine.add(w)
                if w < nwords:
                    marks[w] = v
            for slot in range(first[i], first[i + 1]):
                lo_raw, hi_raw = lo_in[slot], hi_in[slot]               # (before any store)
                if lo_raw == NONE:                                      # touches neither text nor marks
                    out[slot] = NONE
                    if on_none is not None:
                        on_none[slot] = NONE
                    continue
                lo = min(lo_raw, e - b)
                hi = min(max(hi_raw, lo), e - b)
                gl, gh = b + lo, b + hi
                assert b <= gl <= gh <= e
                before = set(mine)
                mine.clear()
                # ---- backward
                st, acc, q = r_start, 0, gh
                while True:
                    bit = (q - base) & 31
                    if r_acc[st]:
                        acc |= 1 << bit
                    if bit == 0:
                        put(word_of(q), acc)
                        acc = 0
                    if q == gl or st == 0:
                        break
                    q -= 1
                    st = r_next[st][r_cls[text[q]]]
                if q > gl:
                    if (q - base) & 31:
                        put(word_of(q), acc)
                    for w in range(word_of(q) - 1, word_of(gl) - 1, -1):
                        put(w, 0)
                elif (gl - base) & 31:
                    put(word_of(gl), acc)
                assert mine == set(range(word_of(gl), word_of(gh) + 1)), "this slot's backward phase stores every word of its own stretch"
                self.shared_words += len(mine & before)
                # ---- forward: the cached mark word starts empty, every word it reads is one this slot stored
                marked = lambda g: (marks[word_of(g)] >> ((g - base) & 31)) & 1 if word_of(g) < nwords else 0
                st, p, answer = f_start, gl, NONE
                if f_acc[st] and marked(gl):
                    answer = lo
                while p < gh and st != 0:
                    st = f_next[st][f_cls[text[p]]]
                    p += 1
                    if f_acc[st] and marked(p):
                        answer = p - b
                mine |= before
                out[slot] = answer
                if answer == NONE and on_none is not None:
                    on_none[slot] = NONE
        return stored

    def run_list(self, items, lists, trim=0, lead=0, first0=0, in_place=False):
        """The launches of rrx_group_spans_list_* on one batch -> [[(start, end) per match] per item]; the marks' properties asserted."""
        self.shared_words = getattr(self, "shared_words", 0)
        text, offs = pack(items, trim, lead, seed=len(items))
        text = text.tolist()
        n, base = len(items), int(offs[0])
        words = marks_words(int(offs[-1]) - base, n)
        marks = [POISON] * (words + 64)
        first, in_start, in_end = csr_lists([[(s & NONE, e & NONE) for s, e in w] for w in lists], first0)
        slots = len(in_start)
        in_start = [POISON if x is None else x for x in in_start]       # the slots below first[0] belong to somebody else
        in_end = [POISON if x is None else x for x in in_end]
        d_start, d_end = (in_start, in_end) if in_place else ([POISON] * slots, [POISON] * slots)
        written = lambda arr: all((arr[q] != POISON) == (q >= first0) for q in range(slots))
        # the copies of the absent parts come first, over the slot range
        for q in range(first0, slots):
            if not self.has_a:
                d_start[q] = in_start[q]
            if not self.has_c:
                d_end[q] = in_end[q]
        touched = {}
        if self.has_a:
            for i, w in self.launch_list(text, offs, trim, first, in_start, in_end, rr.PROGRAM_GROUP_REV_BC, rr.PROGRAM_GROUP_A, marks, words, d_start, d_end).items():
                touched.setdefault(i, set()).update(w)
        if self.has_c:
            lo = d_start if self.has_a else in_start
            for i, w in self.launch_list(text, offs, trim, first, lo, in_end, rr.PROGRAM_GROUP_REV_C, rr.PROGRAM_GROUP_B, marks, words, d_end, d_start).items():
                touched.setdefault(i, set()).update(w)
        assert written(d_start) and written(d_end), "exactly the slots first[0] .. first[n] are written"
        # no word of another item touched: item i's words lie inside its own range, the ranges of two items do not meet
        for i, w in touched.items():
            b, e = self.span(offs, i, trim)
            assert all(((b - base) >> 5) + i <= x <= ((e - base) >> 5) + i for x in w), (i, "a word outside the item's own range")
        owners = [w for w in touched.values() if w]
        assert sum(len(w) for w in owners) == len(set().union(*owners)) if owners else True, "two items share a word"
        everything = set().union(*owners) if owners else set()
        assert not everything or max(everything) < words, "the largest index lies below the bound"
        assert all(marks[w] == POISON for w in range(len(marks)) if w not in everything)
        assert all((d_start[q] == NONE) == (d_end[q] == NONE) for q in range(first0, slots))
        pair = lambda q: (-1, -1) if d_start[q] == NONE else (d_start[q], d_end[q])
        return [[pair(q) for q in range(first[i], first[i + 1])] for i in range(n)]


def test_list_spans_replay_against_the_brute_force():
    slots = none = shared = multi = 0
    for p, ngroups, items, lists, spans in reference_templates():
        assert any(len(w) >= 2 for w in lists) and any(not w for w in lists) or rr.RRegex(p).accepts_empty, p
        for g in range(1, ngroups + 1):
            rep = ListReplay(rr.RGroup(p, g))
            for n_run, (trim, lead, first0, in_place) in enumerate(((0, 5, 0, False), (1, 37, 3, True))):      # base != 0, both trims, d_first[0] != 0, in place
                got = rep.run_list(list(items), lists, trim, lead, first0, in_place)
                for k, (gk, wk) in enumerate(zip(got, spans[g])):
                    assert gk == list(wk), (p, g, k, items[k], lists[k], gk, wk)
            shared += rep.shared_words
            # the first match of an item: test_group_items_lowering's own brute force
            for it, w, sp in zip(items, lists, spans[g]):
                assert (sp[0] if w else (-1, -1)) == group_brute_force(p, g, it), (p, g, it)
                slots += len(w)
                multi += len(w) >= 2
                none += sum(x == (-1, -1) for x in sp)
    print("slots", slots, "items with two matches and more", multi, "mark words shared by consecutive slots", shared)
    assert slots > 1500 and multi > 300 and shared > 300 and none == 0         # (a true match always has a split)


def test_list_spans_of_wild_lists():
    """Slots that are no matches report none, a start of ~0u is passed on, spans beyond the item are clamped; adjacent matches and
    the 33 matches of one item share their mark words."""
    p = "([0-9]+)-([0-9]+)"
    items = [b"x 12-345 y", b"12-3", b"", b"12-3 4-5"]
    lists = [[(0, 5), (2, 8)], [(-1, -1), (0, 4), (1, 4), (1, 0xFFFFFFF0)], [], [(0, 4), (5, 8)]]
    # (group 2 has no C: its end is the list's own, copied as rrx_group_spans_extents copies it - the template passes clamp it)
    for g, want in ((2, [[(-1, -1), (5, 8)], [(-1, -1), (3, 4), (3, 4), (3, 0xFFFFFFF0)], [], [(3, 4), (7, 8)]]),
                    (1, [[(-1, -1), (2, 4)], [(-1, -1), (0, 2), (1, 2), (1, 2)], [], [(0, 2), (5, 6)]])):
        rep = ListReplay(rr.RGroup(p, g))
        assert rep.run_list(items, lists, trim=1, lead=3, first0=2) == want, g
        assert rep.run_list(items, lists, trim=0, lead=0, in_place=True) == want, g
    # 33 adjacent matches in one item, each sharing the bit of e_k == s_{k+1} with its neighbour
    p, item = "(a)(b*)", b"ab" * 20 + b"a" * 13
    lists = [all_longest_brute_force(oracles_for(p, 1)[0].o, item[:MAX_ITEM])]
    assert all(e == s2 for (_, e), (s2, _) in zip(lists[0], lists[0][1:])) and len(lists[0]) >= 11
    long_list = [(m.start(), m.end()) for m in re.finditer(rb"ab*", item)]
    assert len(long_list) == 33 and long_list[:len(lists[0]) - 1] == lists[0][:-1]
    for g in (1, 2):
        rep = ListReplay(rr.RGroup(p, g))
        got = rep.run_list([b"", item, b""], [[], long_list, []], trim=1, lead=31, first0=1)
        assert got[1] == [m.span(g) for m in re.finditer(rb"(a)(b*)", item)]
        assert rep.shared_words >= 32


# ------------------------------------------------------------------------------------------------ sizes and fill
def device_program(segs, refs):
    """The segment program as the kernels take it: (kind, literal offset, literal length) per segment, and the literals."""
    prog, lits = [], b""
    for s in segs:
        if isinstance(s, bytes):
            prog.append((0, len(lits), len(s)))
            lits += s
        else:
            prog.append((1 if s == 0 else 2 + refs.index(s), 0, 0))
    return prog, lits


def walk(prog, slot, L, start, end, ref_start, ref_end, stride, d):
    """walk_template: -> (length so far, None) if no segment holds byte d, else (_, (literal?, begin, end, src))."""
    run = 0
    for kind, lit_off, lit_len in prog:
        if kind == 0:
            src, n = lit_off, lit_len
        else:
            s, e = (start[slot], end[slot]) if kind == 1 else (ref_start[(kind - 2) * stride + slot], ref_end[(kind - 2) * stride + slot])
            if s == NONE:
                continue
            s1 = min(s, L)
            e1 = min(max(e, s1), L)
            src, n = s1, e1 - s1
        if d is not None and d - run < n:
            return run, (kind == 0, run, run + n, src)
        run += n
    return run, None


def sizes_replay(prog, offs, trim, first, start, end, ref_start, ref_end, stride):
    """replace_template_sizes_kernel: a lane per item -> (d_len[n], d_pos by slot; None where the kernel stores nothing)."""
    length, pos = [], [None] * len(start)
    for i in range(len(offs) - 1):
        b, e = span(offs, i, trim)
        shift = 0
        for slot in range(first[i], first[i + 1]):
            assert pos[slot] is None
            pos[slot] = (start[slot] + shift) & 0xffffffff
            shift = (shift + walk(prog, slot, e - b, start, end, ref_start, ref_end, stride, None)[0] - (end[slot] - start[slot])) & M64
        total = (e - b + shift) & M64
        if total >> 63:
            total = 0
        length.append(min(total, 0xffffffff))
    return length, pos


class TemplateFillReplay:
    """replace_template_fill_kernel on a batch: test_replace_items_lowering's FillReplay with the segment level in locate."""

    def __init__(self, text, offs, trim, first, start, end, pos, prog, lits, ref_start, ref_end, stride, out_off, out, out_addr):
        self.text, self.offs, self.trim, self.first, self.start, self.end, self.pos = text, offs, trim, first, start, end, pos
        self.prog, self.lits, self.ref_start, self.ref_end, self.stride = prog, lits, ref_start, ref_end, stride
        self.out_off, self.out, self.out_addr = out_off, out, out_addr
        self.written = bytearray(len(out))
        self.dword_stores = self.byte_stores = self.locates = self.segment_hits = self.tails = 0
        self.boundaries = set()                                     # (address of a segment's first output byte) mod 4

    def store(self, at, value, width):
        assert 0 <= at and at + width <= len(self.out)
        for k in range(width):
            assert not self.written[at + k], ("a byte stored twice", at + k)
            self.written[at + k] = 1
            self.out[at + k] = (value >> (8 * k)) & 0xff

    def run(self):
        n = len(self.offs) - 1
        for F in range(0, n, 64):
            self.wave_pass(F, n)

    def wave_pass(self, F, n):
        row = [self.out_off[min(F + lane, n)] for lane in range(64)] + [self.out_off[min(F + 64, n)]]
        lo, hi = row[0], row[64]
        if hi <= lo:
            return
        mis = (self.out_addr + lo) & 3
        total = hi - lo + mis
        pos, first = self.pos, self.first
        for rel in range(0, total, 4):
            c0 = mis - rel if rel < mis else 0
            c1 = min(total - rel, 4)
            lim, word = -1, 0
            for c in range(c0, c1):
                q = lo + rel + c - mis
                if c == c0 or q >= lim:                             # locate(q)
                    self.locates += 1
                    idx, step = 0, 32
                    while step:
                        if row[idx + step] <= q:
                            idx += step
                        step >>= 1
                    o0, o1 = row[idx], row[idx + 1]
                    assert o0 <= q < o1 and F + idx < n
                    r = q - o0
                    b, e = span(self.offs, F + idx, self.trim)
                    item_len = e - b
                    f0, f1 = first[F + idx], first[F + idx + 1]
                    below, above = f0, max(f0, f1)
                    while below < above:
                        mid = below + ((above - below) >> 1)
                        if pos[mid] <= r:
                            below = mid + 1
                        else:
                            above = mid
                    lim = o1
                    if below < f1:
                        lim = min(lim, o0 + pos[below])
                    in_lit, origin = False, o0
                    if below > f0:
                        j = below - 1
                        at = o0 + pos[j]
                        rep_len, hit = walk(self.prog, j, item_len, self.start, self.end, self.ref_start, self.ref_end, self.stride, q - at)
                        if hit is not None:
                            in_lit, begin, seg_end, src = hit
                            origin = (at + begin - src) & M64
                            lim = min(lim, at + seg_end)
                            self.segment_hits += 1
                            if q == at + begin:
                                self.boundaries.add((self.out_addr + q) & 3)
                        else:
                            origin = (at + rep_len - self.end[j]) & M64
                            self.tails += 1
                    assert lim > q
                src = (q - origin) & M64
                if in_lit:
                    v = self.lits[src]
                else:
                    v = self.text[b + src] if src < item_len else 0   # no byte outside the item is read
                word |= v << (8 * c)
            dst = lo + rel - mis
            assert (self.out_addr + dst) % 4 == 0
            if c0 == 0 and c1 == 4:
                self.dword_stores += 1
                self.store(dst, word, 4)
            else:
                for c in range(c0, c1):
                    self.byte_stores += 1
                    self.store(dst + c, (word >> (8 * c)) & 0xff, 1)


def flat_planes(spans, refs, first, nslots, stride):
    """{g: [[(i, j) per match] per item]} -> (ref_start, ref_end): plane r, slot q at r * stride + q; everything else poisoned."""
    rs, re_ = [POISON] * (len(refs) * stride + 1), [POISON] * (len(refs) * stride + 1)
    for r, g in enumerate(refs):
        for i, w in enumerate(spans[g]):
            for k, (s, e) in enumerate(w):
                rs[r * stride + first[i] + k], re_[r * stride + first[i] + k] = s & NONE, e & NONE
    return rs, re_


def replay(items, lists, spans, repl, trim=0, lead=0, out_first=0, out_addr=0, first0=0, extra_stride=0):
    """One batch through both kernels -> (the output items, the TemplateFillReplay for its counters)."""
    segs = parse_py(repl)
    refs = sorted({s for s in segs if isinstance(s, int) and s > 0})
    prog, lits = device_program(segs, refs)
    text, offs = pack(items, trim, lead, seed=len(items))
    text = text.tolist()
    n = len(items)
    first, start, end = csr_lists(lists, first0)
    stride = len(start) + extra_stride
    ref_start, ref_end = flat_planes(spans, refs, first, len(start), stride)
    length, pos = sizes_replay(prog, offs, trim, first, start, end, ref_start, ref_end, stride)
    assert all((p is None) == (slot < first0) for slot, p in enumerate(pos)), "exactly the slots first[0] .. first[n] are stored"
    out_off = [out_first]
    for x in length:
        out_off.append(out_off[-1] + x)
    out = bytearray([OUT_POISON]) * (out_off[-1] + MARGIN)
    f = TemplateFillReplay(text, offs, trim, first, start, end, pos, prog, lits, ref_start, ref_end, stride, out_off, out, out_addr)
    f.run()
    assert all(f.written[out_first:out_off[-1]]) and not any(f.written[:out_first]) and not any(f.written[out_off[-1]:]), "exactly [out_off[0], out_off[n])"
    return [bytes(out[out_off[i]:out_off[i + 1]]) for i in range(n)], f


def test_sizes_and_fill_replay_against_the_splice():
    hits = tails = out_bytes = dwords = singles = 0
    boundaries = set()
    for n_p, (p, ngroups, items, lists, spans) in enumerate(reference_templates()):
        for n_t, repl in enumerate(TEMPLATES):
            if any(isinstance(s, int) and s > ngroups for s in parse_py(repl)):
                continue
            want = expected_items(items, lists, spans, repl)
            for trim, lead in ((0, 5), (1, 37)):
                got, f = replay(list(items), lists, spans, repl, trim=trim, lead=lead, out_first=(n_p + trim) % 7, out_addr=(n_p + n_t + trim) % 4,
                                first0=n_p % 3, extra_stride=n_t % 2 * 5)
                assert got == want, (p, repl, next(k for k in range(len(got)) if got[k] != want[k]))
                hits, tails, out_bytes, dwords, singles = hits + f.segment_hits, tails + f.tails, out_bytes + sum(map(len, got)), dwords + f.dword_stores, singles + f.byte_stores
                boundaries |= f.boundaries
            if repl == rb"\0":                                      # the column without its separators
                assert want == list(items)
            if b"\\" not in repl:                                   # a literal: the literal kernels' rule
                assert want == [splice(it, w, repl) for it, w in zip(items, lists)]
    print("output bytes", out_bytes, "dword stores", dwords, "byte stores", singles, "segment hits", hits, "tails", tails)
    assert out_bytes == 4 * dwords + singles and hits > 1000 and tails > 1000 and boundaries == {0, 1, 2, 3}


def test_against_re_sub():
    """Where test_group_items_lowering shows that Python's rule is ours (its NAMED cases) and Python's greedy search names the
    leftmost-longest list, the replay on re.finditer's list and spans is re.sub with the template translated: \\0 -> \\g<0>, a
    reference followed by a digit -> \\g<n>."""
    translate = lambda repl: re.sub(rb"\\([0-9])", lambda m: b"\\g<" + m.group(1) + b">", repl)
    assert translate(rb"[\12]\0\\") == rb"[\g<1>2]\g<0>\\"
    for p, g, item, want in NAMED[:4]:
        assert re.search(p.encode(), item).span(g) == want
    rng = random.Random(SEED + 32)
    for p, ngroups, alphabet in ((DATE, 3, "0199/ x"), ("([0-9]+)-([0-9]+)", 2, "019- x"), ("[a-z]*([0-9]+)[0-9]", 1, "ab019 "), ("https?://([^/]+)/.*", 1, "htps:/ab.")):
        rx = re.compile(p.encode())
        items = ["".join(rng.choice(alphabet) for _ in range(rng.randrange(MAX_ITEM + 1))).encode() for _ in range(100)]
        items += [b"1/2/3 10/20/1999x", b"12-3 4-56", b"ab123 c45", b"see http://a.b/c"]
        whole = oracles_for(p, 1)[0]
        lists = [all_longest_brute_force(whole.o, it) for it in items]
        assert lists == [[m.span() for m in rx.finditer(it)] for it in items], p
        spans = {g: [[span_group(p, g, it, s, e) for s, e in w] for it, w in zip(items, lists)] for g in range(1, ngroups + 1)}
        assert all(spans[g] == [[m.span(g) for m in rx.finditer(it)] for it in items] for g in spans), p
        items += [b" ".join(rng.choice(items[:8] + items[-4:] * 2) for _ in range(rng.randrange(20, 50))) for _ in range(10)]      # beyond the brute force: Python's spans
        lists = [[m.span() for m in rx.finditer(it)] for it in items]
        spans = {g: [[m.span(g) for m in rx.finditer(it)] for it in items] for g in range(1, ngroups + 1)}
        assert sum(len(w) for w in lists) > 10 and (".*" in p or sum(len(w) for w in lists) > 50), p     # (.* runs to the item's end: a match per item)
        for repl in TEMPLATES:
            if any(isinstance(s, int) and s > ngroups for s in parse_py(repl)):
                continue
            got, _ = replay(items, lists, spans, repl, trim=1, lead=3, out_first=5, out_addr=len(repl) % 4, first0=1)
            assert got == [rx.sub(translate(repl), it) for it in items], (p, repl)
    assert re.sub(rb"([0-9]+)/([0-9]+)/([0-9]+)", rb"\3-\1-\2", b"on 12/31/1999.") == b"on 1999-12-31."


def test_wild_spans_read_no_byte_outside_the_item():
    """Planes and lists of another batch: every byte of [out_off[0], out_off[n]) is still written once and nothing else, both passes
    agree on every length (the fill asserts lim > q and finds its bytes), and the replay reads text[b + src] only for src < the item's
    length.  A start of ~0u contributes nothing; a span beyond the item is clamped."""
    rng = random.Random(SEED + 33)
    items = [bytes(rng.choice(b"abc") for _ in range(rng.randrange(12))) for _ in range(100)]
    lists = [sorted((s, s + rng.randrange(3)) for s in rng.sample(range(0, 30, 3), rng.randrange(3))) for _ in items]
    wild = lambda: (rng.choice([NONE, 0, 3, 40, 0xFFFFFFF0]), rng.choice([0, 2, 7, 50, NONE]))
    spans = {g: [[wild() for _ in w] for w in lists] for g in (1, 2)}
    text, offs = pack(items, 1, 3)
    segs = parse_py(rb"<\1|\2|\0>")
    prog, lits = device_program(segs, [1, 2])
    first, start, end = csr_lists(lists)
    stride = len(start) + 3
    ref_start, ref_end = flat_planes(spans, [1, 2], first, len(start), stride)
    length, pos = sizes_replay(prog, offs, 1, first, start, end, ref_start, ref_end, stride)
    out_off = [2]
    for x in length:
        out_off.append(out_off[-1] + x)
    out = bytearray([OUT_POISON]) * (out_off[-1] + MARGIN)
    f = TemplateFillReplay(text.tolist(), offs, 1, first, start, end, pos, prog, lits, ref_start, ref_end, stride, out_off, out, 3)
    f.run()
    assert all(f.written[2:out_off[-1]]) and not any(f.written[:2]) and not any(f.written[out_off[-1]:])
    # the replacement of a slot, by the rule: clamped spans, ~0u contributes nothing
    k = next(i for i, w in enumerate(lists) if w and lists[i][0][1] <= len(items[i]))
    it, L = items[k], len(items[k])
    clamp = lambda s, e: b"" if s == NONE else it[min(s, L):min(max(e, min(s, L)), L)]
    s0, e0 = lists[k][0]
    want = b"<" + clamp(*spans[1][k][0]) + b"|" + clamp(*spans[2][k][0]) + b"|" + it[s0:e0] + b">"
    got = bytes(out[out_off[k]:out_off[k + 1]])
    assert got[s0:s0 + len(want)] == want, (it, lists[k], got, want)
