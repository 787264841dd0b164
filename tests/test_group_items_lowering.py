"""regexp_extract with a capture group (rrx_group_* / rrx_extract_group_longest_*) on the CPU: the splitter (rrx_group_part and the
return codes of rrx_group_compile), the split's faithfulness - the oracle of the whole pattern accepts w iff the oracles of the
three part texts accept some w[:i], w[i:j], w[j:] -, and the four tables (RRX_PROGRAM_GROUP_*) replayed BATCH BY BATCH as
longest_split_kernel is specified: backward on the reverse table from hi down to lo, the mark bits of 32 consecutive offsets gathered
and stored as the walk crosses a mark-word boundary downwards and once more at lo, zero words without the text behind the dead row,
into ONE flat marks array of the whole batch (word ((g - base) >> 5) + i, bit (g - base) & 31, the stretch's end included); then
forward on the forward table, the last marked accepting offset - launched twice, on (reverse (B)C, A) over the whole match and on
(reverse C, B) over [i, e] - against a brute force of the header's SEMANTICS built from test_search_longest_items_lowering's
longest_brute_force and the parts' oracles.  Also the entries' argument checks, which need no device."""
import functools
import random
import re

import pytest

import roaringregex_amd as rr
from program_replay import DfaReplay
from pyoracle import OracleRegex
from test_contains_items_lowering import MAX_ITEM, short_items
from test_search_all_longest_items_lowering import POISON, pack
from test_search_longest_items_lowering import SEED, longest_brute_force

OK, PATTERN, ARG, UNSUPPORTED = 0, 1, 2, 4
NONE = 0xFFFFFFFF
marks_words = rr._L.rrx_search_all_longest_marks_words
POSIX_DIVERGENT = ("(a|ab)(c|bcd)?(d*)", 3)
GLOBAL_A = "[ab]*a[ab]{12}x(c+)d*"                  # A's table alone (8192 subsets and more) is beyond 64 KiB: that launch runs from HBM/L2
# (pattern, group): the random part.  The last eight are ambiguous on purpose: many items admit several i or several j.
RANDOM_CASES = (("https?://([^/]+)/.*", 1), ("([0-9]+)-([0-9]+)", 1), ("([0-9]+)-([0-9]+)", 2), ("[a-z]*([0-9]+)[0-9]", 1), ("x(a*)", 1), ("(a+)", 1),
                ("a((b)c)d", 1), ("[(]x(y)z*", 1), ("a\\(b\\)(c+)c", 1), ("(ab|a)(bc|c)?", 1), ("(a|b)*(ab?)(b|c)*", 2), ("a*(a*)a*", 1), POSIX_DIVERGENT,
                ("[a-c]*([a-c]+)[a-c]*", 1), ("[ab]*(a[ab]*)b[ab]*", 1), ("[a-c]+([a-c]*)", 1), ("(a+)a*b?", 1), ("[xy]*([xy]+)y*", 1),
                ("[ab]+(b*)[ab]+", 1))
ALPHABETS = {"https?://([^/]+)/.*": "htps:/ab.", "([0-9]+)-([0-9]+)": "019- x", "[a-z]*([0-9]+)[0-9]": "ab019 ", "x(a*)": "xab", "(a+)": "ab",
             "a((b)c)d": "abcd", "[(]x(y)z*": "(xyz", "a\\(b\\)(c+)c": "a(b)c", "(ab|a)(bc|c)?": "abc", "(a|b)*(ab?)(b|c)*": "abcx", "a*(a*)a*": "aab",
             POSIX_DIVERGENT[0]: "abcd", "[a-c]*([a-c]+)[a-c]*": "abcx", "[ab]*(a[ab]*)b[ab]*": "abx", "[a-c]+([a-c]*)": "abcx",
             "(a+)a*b?": "aab", "[xy]*([xy]+)y*": "xyz", "[ab]+(b*)[ab]+": "abx"}
# matches planted into one item in four, so that patterns a random item hardly ever contains show both verdicts
PLANTS = {"https?://([^/]+)/.*": (b"http://a.b/", b"https://h/ab/", b"http:///", b"http://p/"), "([0-9]+)-([0-9]+)": (b"1-0", b"90-11-9"),
          "[a-z]*([0-9]+)[0-9]": (b"ab10", b"199"), "a((b)c)d": (b"abcd",), "[(]x(y)z*": (b"(xy", b"(xyzz"), "a\\(b\\)(c+)c": (b"a(b)cc", b"a(b)cccc"),
          "(a|b)*(ab?)(b|c)*": (b"ababcb",), POSIX_DIVERGENT[0]: (b"abcd", b"abcdd", b"acdd")}
# the named cases of the header and the issue: (pattern, group, item, answer)
NAMED = (("https?://([^/]+)/.*", 1, b"see http://example.com/a/b", (11, 22)), ("([0-9]+)-([0-9]+)", 1, b"x 12-345 y", (2, 4)),
         ("([0-9]+)-([0-9]+)", 2, b"x 12-345 y", (5, 8)), ("[a-z]*([0-9]+)[0-9]", 1, b"ab1234", (2, 5)), ("a*(a*)a*", 1, b"aaaa", (4, 4)),
         POSIX_DIVERGENT + (b"abcd", (4, 4)))


def compile_code(p, group):
    """(return code of rrx_group_compile, error text) - the handle freed again."""
    h = rr.C.c_void_p()
    rc = rr._L.rrx_group_compile(p.encode("latin-1") if isinstance(p, str) else p, group, rr.C.byref(h))
    err = rr._L.rrx_last_error()
    assert bool(h.value) == (rc == OK)
    if h.value:
        rr._L.rrx_group_free(h)
    return rc, err


class Part:
    """The oracle of a part's source text; an absent part accepts the empty word alone ("" itself lexes to an atom, not to it)."""

    def __init__(self, text):
        self.o = OracleRegex(text.decode("latin-1")) if text else None
        self.memo = {}

    def accepts(self, w):
        if self.o is None:
            return not w
        if w not in self.memo:
            self.memo[w] = bool(self.o.accepts(w))
        return self.memo[w]


@functools.lru_cache(maxsize=None)
def oracles_for(p, group):
    """(whole, A, B, C): the oracle of the pattern and of the three part texts rrx_group_part names."""
    g = rr.RGroup(p, group)
    return (Part(p.encode("latin-1")),) + tuple(Part(t) for t in g.parts)


def admissible(p, group, item):
    """(s, e, the admissible i, the admissible j for the largest i) of the header's SEMANTICS; None without a match."""
    whole, a, b, c = oracles_for(p, group)
    s, e = longest_brute_force(whole, item)
    if e < 0:
        return None
    bc = lambda i: [j for j in range(i, e + 1) if b.accepts(item[i:j]) and c.accepts(item[j:e])]
    i_s = [i for i in range(s, e + 1) if a.accepts(item[s:i]) and bc(i)]
    assert i_s, ("a match of the whole pattern without a split", p, item, s, e)
    return s, e, i_s, bc(max(i_s))


def group_brute_force(p, group, item):
    adm = admissible(p, group, item)
    return (-1, -1) if adm is None else (max(adm[2]), max(adm[3]))


def items_for(p, rng, n):
    """Short items over the pattern's own alphabet, empty ones among them, and short_items' mix (NUL, high bytes, '\\n')."""
    a = ALPHABETS[p]
    items = ["".join(rng.choice(a) for _ in range(rng.choice([0, 1, 3, 5, 8, 12, 17, MAX_ITEM]))).encode() for _ in range(n)]
    for k in range(2, n, 4):
        if p in PLANTS:
            plant, at = rng.choice(PLANTS[p]), rng.randint(0, len(items[k]))
            items[k] = (items[k][:at] + plant + items[k][at:])[:MAX_ITEM]
    items[3] = items[n // 2] = b""
    return items + short_items(rng, "ab", 40)[:24]


@functools.lru_cache(maxsize=None)
def reference_groups():
    """[(pattern, group, items, want)]: computed once (the device tests share it), never changed."""
    rng = random.Random(SEED + 21)
    out = []
    for p, g in RANDOM_CASES:
        items = tuple(items_for(p, rng, 120))
        out.append((p, g, items, tuple(group_brute_force(p, g, it) for it in items)))
    return tuple(out)


class GroupReplay:
    """longest_split_kernel on a batch, in Python ints, and the two launches of the entries around it."""

    def __init__(self, g):
        self.parts = g.parts
        self.has_a, self.has_c = bool(self.parts[0]), bool(self.parts[2])
        self.tables = {}
        for kind in (rr.PROGRAM_GROUP_A, rr.PROGRAM_GROUP_REV_BC, rr.PROGRAM_GROUP_B, rr.PROGRAM_GROUP_REV_C):
            w = g.program(kind)
            if w is None:
                continue
            d = DfaReplay(w)
            t = (d.cls.tolist(), d.next.tolist(), d.acc.tolist(), d.start)
            assert not t[2][0] and not any(t[1][0]), "row 0 must be dead and absorbing: both passes stop there"
            self.tables[kind] = t
        assert (rr.PROGRAM_GROUP_A in self.tables) == (rr.PROGRAM_GROUP_REV_BC in self.tables) == self.has_a
        assert (rr.PROGRAM_GROUP_REV_C in self.tables) == self.has_c and rr.PROGRAM_GROUP_B in self.tables
        self.dead_fills = self.early_exits = 0

    @staticmethod
    def span(offs, i, trim):
        b, e = int(offs[i]), int(offs[i + 1])
        return b, (e - trim if e - b >= trim else b)

    def launch(self, text, offs, trim, lo_in, hi_in, rev, fwd, marks, nwords):
        """One launch on the whole batch -> (out, the set of words an item had to store).  Asserts: no word stored twice."""
        r_cls, r_next, r_acc, r_start = self.tables[rev]
        f_cls, f_next, f_acc, f_start = self.tables[fwd]
        base, n = int(offs[0]), len(offs) - 1
        owner, expected, out = {}, set(), []
        for i in range(n):
            if lo_in[i] == NONE:                                    # touches neither text nor marks
                out.append(NONE)
                continue
            b, e = self.span(offs, i, trim)
            lo = min(lo_in[i], e - b)
            hi = min(max(hi_in[i], lo), e - b)
            gl, gh = b + lo, b + hi
            assert b <= gl <= gh <= e
            word_of = lambda g: ((g - base) >> 5) + i
            expected |= set(range(word_of(gl), word_of(gh) + 1))

            def put(w, v):
                assert w not in owner, ("word stored twice", w, owner[w], i)
                owner[w] = i
                if w < nwords:
                    marks[w] = v
            # ---- backward
            st, acc, q = r_start, 0, gh
            while True:                                             # offset q gets its mark
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
            if q > gl:                                              # dead above lo: the words left, without the text
                self.dead_fills += 1
                if (q - base) & 31:
                    put(word_of(q), acc)
                for w in range(word_of(q) - 1, word_of(gl) - 1, -1):
                    put(w, 0)
            elif (gl - base) & 31:
                put(word_of(gl), acc)
            # ---- forward
            marked = lambda g: (marks[word_of(g)] >> ((g - base) & 31)) & 1 if word_of(g) < nwords else 0
            st, p, answer = f_start, gl, NONE
            if f_acc[st] and marked(gl):
                answer = lo
            while p < gh:
                if st == 0:
                    self.early_exits += 1
                    break
                st = f_next[st][f_cls[text[p]]]
                p += 1
                if f_acc[st] and marked(p):
                    answer = p - b
            out.append(answer)
        assert set(owner) == expected, "every word of every [lo, hi] range, and no other"
        return out, expected

    def run(self, items, spans, trim=0, lead=0, true_matches=True):
        """The two launches on one batch, from the span list `spans` ((-1, -1): none), the layout's properties asserted after each
        -> [(start, end)].  true_matches: the spans are matches of the whole pattern - each must yield a split."""
        text, offs = pack(items, trim, lead, seed=len(items))
        text = text.tolist()
        n, base = len(items), int(offs[0])
        words = marks_words(int(offs[-1]) - base, n)
        marks = [POISON] * (words + 64)
        start = [s & NONE for s, _ in spans]
        end = [e & NONE for _, e in spans]
        stored = set()
        if self.has_a:
            out, touched = self.launch(text, offs, trim, start, end, rr.PROGRAM_GROUP_REV_BC, rr.PROGRAM_GROUP_A, marks, words)
            assert not touched or max(touched) < words, (max(touched), words)
            end = [NONE if o == NONE else x for o, x in zip(out, end)]
            start = out
            stored |= touched
        if self.has_c:
            out, touched = self.launch(text, offs, trim, start, end, rr.PROGRAM_GROUP_REV_C, rr.PROGRAM_GROUP_B, marks, words)
            assert not touched or max(touched) < words, (max(touched), words)
            start = [NONE if o == NONE else x for o, x in zip(out, start)]
            end = out
            stored |= touched
        assert all(marks[w] == POISON for w in range(len(marks)) if w not in stored), "a word outside the items' ranges was touched"
        got = [(-1, -1) if s == NONE or e == NONE else (s, e) for s, e in zip(start, end)]
        assert all((s == NONE) == (e == NONE) for s, e in zip(start, end))
        if true_matches:
            assert all((g == (-1, -1)) == (sp[0] < 0) for g, sp in zip(got, spans)), "a true whole match always yields a split"
        return got


def check(p, group, items, want, trim=0, lead=0):
    whole = oracles_for(p, group)[0]
    rep = GroupReplay(rr.RGroup(p, group))
    got = rep.run(list(items), [longest_brute_force(whole, it) for it in items], trim, lead)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == tuple(w), (p, group, k, items[k], g, w)
    return rep


# ------------------------------------------------------------------------------------------------ the splitter
def test_parts():
    assert rr.RGroup("https?://([^/]+)/.*", 1).parts == (b"https?://", b"[^/]+", b"/.*")
    assert rr.RGroup("([0-9]+)-([0-9]+)", 1).parts == (b"", b"[0-9]+", b"-([0-9]+)")
    assert rr.RGroup("([0-9]+)-([0-9]+)", 2).parts == (b"([0-9]+)-", b"[0-9]+", b"")
    assert rr.RGroup("[(]x(y)", 1).parts == (b"[(]x", b"y", b"")                 # a '(' inside brackets is no group
    assert rr.RGroup("a\\(b\\)(c)", 1).parts == (b"a\\(b\\)", b"c", b"")          # nor is an escaped one
    assert rr.RGroup("a((b)c)d", 1).parts == (b"a", b"(b)c", b"d")               # nested ones count: group 2 is (b)
    g = rr.RGroup("(ab)", 1)
    assert g.parts == (b"", b"ab", b"") and g.regex.pattern == b"(ab)" and g.regex.states_n == rr.RRegex("(ab)").states_n
    # rrx_group_part writes nothing past cap and returns the length
    buf = rr.C.create_string_buffer(b"#" * 8)
    assert rr._L.rrx_group_part(rr.RGroup("https?://([^/]+)/.*", 1)._h, 0, buf, 3) == 9 and buf.raw[:8] == b"htt#####"
    assert rr._L.rrx_group_part(g._h, 3, buf, 8) == 0 and rr._L.rrx_group_part(None, 0, buf, 8) == 0


def test_return_codes():
    rc, err = compile_code("a((b)c)d", 2)
    assert rc == UNSUPPORTED and b"nested" in err
    assert compile_code("a((b)c)d", 1)[0] == OK
    rc, err = compile_code("(a)|b", 1)
    assert rc == UNSUPPORTED and b"'|'" in err
    for p, mark in (("(ab)+c", b"'+'"), ("(ab){2}c", b"'{'"), ("(ab)?c", b"'?'"), ("(ab)*c", b"'*'")):
        rc, err = compile_code(p, 1)
        assert rc == UNSUPPORTED and mark in err, (p, err)
    assert compile_code("(a)(b)", 0)[0] == ARG and compile_code("(a)(b)", 3)[0] == ARG and compile_code("(a)(b)", -1)[0] == ARG
    assert compile_code("(a)(b)", 1)[0] == OK and compile_code("(a)(b)", 2)[0] == OK
    assert compile_code("ab", 1)[0] == ARG                                      # no group at all
    for bad in ("a()b", ")", "*(a)"):                                           # the whole pattern does not compile
        with pytest.raises(rr.RRegexError):
            rr.RRegex(bad)
        assert compile_code(bad, 1)[0] == PATTERN, bad
    h = rr.C.c_void_p()
    assert rr._L.rrx_group_compile(None, 1, rr.C.byref(h)) == ARG and rr._L.rrx_group_compile(b"(a)", 1, None) == ARG
    assert rr._L.rrx_group_compile_ex(b"(a)", 1, 99, rr.C.byref(h)) == ARG      # unknown engine
    # a part that explodes under subset construction is refused at compile, not by a device entry
    rc, err = compile_code("((a|b)*a(a|b){40})c", 1)
    assert rc == UNSUPPORTED and b"determinise" in err


def test_tables():
    g = rr.RGroup("https?://([^/]+)/.*", 1)
    for kind, accepted, rejected in ((rr.PROGRAM_GROUP_A, (b"http://", b"https://"), (b"http:/", b"xhttp://", b"")),
                                     (rr.PROGRAM_GROUP_REV_BC, (b"/x", b"ba/x"), (b"x/", b"x", b"")),
                                     (rr.PROGRAM_GROUP_B, (b"a", b"abc."), (b"", b"a/")), (rr.PROGRAM_GROUP_REV_C, (b"/", b"cb/"), (b"", b"a", b"/a"))):
        d = DfaReplay(g.program(kind))
        assert all(d.accepts(w) for w in accepted) and not any(d.accepts(w) for w in rejected), kind
    assert g.program(rr.PROGRAM_SEARCH_STARTS) is None and g.regex.program(rr.PROGRAM_SEARCH_STARTS) is not None
    both_absent = rr.RGroup("(ab)", 1)
    assert [both_absent.program(k) is None for k in (21, 22, 23, 24)] == [True, True, False, True]


# ------------------------------------------------------------------------------------------------ the split is faithful
def test_faithful_split():
    """L(P) = L(A) L(B) L(C) through the oracles of the part TEXTS: guards against the reference parser's precedence quirks."""
    cases = RANDOM_CASES + (("x(a|bc)*(c|d)+(e?)f*", 3), ("(a|b)(c)", 2), ("(a|b)(c)", 1))
    assert len(set(cases)) >= 12
    both = 0
    for p, g in cases:
        whole, a, b, c = oracles_for(p, g)
        rng = random.Random(SEED + 22)
        words = set(items_for(p, rng, 120)) if p in ALPHABETS else {"".join(rng.choice("abcdefx") for _ in range(rng.randrange(9))).encode() for _ in range(300)}
        for w in list(words):                                       # ... and what the pattern accepts of them: the other verdict
            s, e = longest_brute_force(whole, w)
            words.add(w[max(s, 0):max(e, 0)])
        for w in words:
            n = len(w)
            split = any(a.accepts(w[:i]) and b.accepts(w[i:j]) and c.accepts(w[j:]) for i in range(n + 1) for j in range(i, n + 1))
            assert whole.accepts(w) == split, (p, g, w)
            both += split
    assert both > 200, both


# ------------------------------------------------------------------------------------------------ the replay
def test_named_cases():
    for p, g, item, want in NAMED:
        assert group_brute_force(p, g, item[-MAX_ITEM:]) == tuple(x - max(0, len(item) - MAX_ITEM) for x in want), (p, g, item)
        got = GroupReplay(rr.RGroup(p, g)).run([b"", item, b"", item], [(-1, -1), whole_span(p, item), (-1, -1), whole_span(p, item)], trim=1, lead=31)
        assert got == [(-1, -1), want, (-1, -1), want], (p, g, got)
    for p, g, item, want in NAMED[:4]:                              # where Python's rule is ours (checked here, relied on by the device tests)
        assert re.search(p.encode(), item).span(g) == want
    # (Python's backtracking happens to answer [4,4) on the POSIX-divergent case too: a, then bcd; POSIX's [3,4) is ab, c, d)


def whole_span(p, item):
    """The leftmost-longest match of a named item (those beyond the brute force's 22 bytes: their tail, which holds the match)."""
    cut = max(0, len(item) - MAX_ITEM)
    s, e = longest_brute_force(OracleRegex(p), item[cut:])
    assert s >= 0
    return s + cut, e + cut


def test_replay_against_the_brute_force():
    ref = reference_groups()
    assert len(ref) >= 12
    matched = ambiguous = dead = early = 0
    for p, g, items, want in ref:
        assert any(not it for it in items[1:-1]) and any(w[0] >= 0 for w in want) and (rr.RRegex(p).accepts_empty or any(w[0] < 0 for w in want)), (p, g)
        for it in items:
            adm = admissible(p, g, it)
            if adm is not None:
                matched += 1
                ambiguous += len(adm[2]) > 1 or len(adm[3]) > 1
        for trim, lead in ((0, 5), (1, 37)):                        # base != 0, both trims, empty items in between
            rep = check(p, g, items, want, trim=trim, lead=lead)
            dead += rep.dead_fills
            early += rep.early_exits
    print("patterns", len(ref), "matched items", matched, "with more than one admissible i or j", ambiguous, "dead fills", dead, "early exits", early)
    assert matched > 500 and 4 * ambiguous >= matched, (matched, ambiguous)
    assert dead > 0 and early > 0                                   # both exits are exercised


def test_coverage_cases():
    # a nullable B, an absent A, an absent C, both absent, a no-match item, an empty item
    for p, g, items in (("x(a*)", 1, [b"x", b"bxaab", b"", b"aa", b"xa"]), ("(a+)b", 1, [b"aab", b"b", b"", b"baaab"]), ("b(a+)", 1, [b"baa", b"", b"ab"]),
                        ("(ab*)", 1, [b"xabbx", b"", b"b", b"a"]), ("a*(a*)a*", 1, [b"", b"b", b"aaaa"])):
        want = [group_brute_force(p, g, it) for it in items]
        assert any(w[0] >= 0 for w in want) and (p == "a*(a*)a*" or any(w[0] < 0 for w in want))
        check(p, g, items, want)
        check(p, g, items, want, trim=1, lead=33)
    assert group_brute_force("x(a*)", 1, b"x") == (1, 1) and group_brute_force("a*(a*)a*", 1, b"") == (0, 0)
    # the empty language: B has a table, the whole pattern matches nowhere
    assert group_brute_force("a([])b", 1, b"ab") == (-1, -1)


def test_marks_straddle_word_boundaries():
    p, g = "[ab]*(a[ab]*)b[ab]*", 1
    for lead in (0, 1, 30, 31, 32):
        items = [b"x" * k + b"ab" * 3 + b"x" * t for k in (0, 1, 9, 14, 15) for t in (0, 1)] + [b"", b"ab" * 11, b"x" * MAX_ITEM]
        want = [group_brute_force(p, g, it) for it in items]
        check(p, g, items, want, trim=0, lead=lead)
        check(p, g, items, want, trim=1, lead=lead)


def test_spans_that_are_no_matches_and_wild_spans():
    """A span list that is not a match reports no match; spans beyond the item are clamped into it."""
    p, g = "([0-9]+)-([0-9]+)", 2
    rep = GroupReplay(rr.RGroup(p, g))
    items = [b"x 12-345 y", b"12-3", b"", b"12-3"]
    spans = [(0, 5), (0, 4), (0, 0), (1, 4)]                        # not a match, a match, not a match, "2-3"
    assert rep.run(items, spans, trim=1, lead=3, true_matches=False) == [(-1, -1), (3, 4), (-1, -1), (3, 4)]
    rep = GroupReplay(rr.RGroup(p, 1))                              # A absent: the second launch alone refuses it
    spans[3] = (1, 0xFFFFFFF0)                                      # clamped to (1, 4)
    assert rep.run(items, spans, trim=0, lead=0, true_matches=False) == [(-1, -1), (0, 2), (-1, -1), (1, 2)]


def test_tables_beyond_the_lds_budget():
    g = rr.RGroup(GLOBAL_A, 1)
    a, rev = g.program(rr.PROGRAM_GROUP_A), g.program(rr.PROGRAM_GROUP_REV_BC)
    plain_bytes = lambda w: int(w[0]) * int(w[1]) * 2 + 256 + int(w[0])
    assert plain_bytes(a) + plain_bytes(rev) > 65536, (plain_bytes(a), plain_bytes(rev))
    items, want = global_items(random.Random(SEED + 23), 40, MAX_ITEM)
    assert [group_brute_force(GLOBAL_A, 1, it) for it in items] == want
    assert 3 < sum(w[0] >= 0 for w in want) < len(items)
    check(GLOBAL_A, 1, items, want, trim=1, lead=7)


def global_items(rng, n, max_len):
    """Items for GLOBAL_A: junk, a run of 13 to 16 of [ab], x, k >= 0 of c, some d, junk.  Python's search names the answer: a match
    wants an a thirteen or more places before the x and a c behind it, and then the group is the run of c (nobody else takes a c)."""
    items, want = [], []
    for _ in range(n):
        run = "".join(rng.choice("abb") for _ in range(rng.randrange(13, 17)))
        it = ("d" * rng.randrange(2) + run + "x" + "c" * rng.randrange(4) + "d" * rng.randrange(2) + "b" * rng.randrange(2))[:max_len]
        m = re.search(rb"[ab]*a[ab]{12}x(c+)d*", it.encode())
        items.append(it.encode())
        want.append(m.span(1) if m else (-1, -1))
        assert m is None or it[m.start(1) - 1] == "x"
    return items, want


# ------------------------------------------------------------------------------------------------ the entries' argument checks
def test_arguments_are_checked_without_a_device():
    L, C = rr._L, rr.C
    g = rr.RGroup("a(b+)c", 1)
    bare = rr.RGroup("(b+)", 1)                                     # both A and C absent: no launch, no marks
    p = C.cast((C.c_uint64 * 8)(), C.c_void_p)
    # rrx_group_spans_extents(grp, device, bytes, off, nitems, trim, match_start, match_end, marks, marks_words, group_start, group_end, stream)
    assert L.rrx_group_spans_extents(None, 0, None, None, 0, 0, None, None, None, 0, None, None, None) == ARG
    assert b"null" in L.rrx_last_error()
    assert L.rrx_group_spans_extents(g._h, 0, p, None, 5, 0, p, p, p, 6, p, p, None) == ARG          # no offsets
    assert L.rrx_group_spans_extents(g._h, 0, p, p, 5, 0, None, p, p, 6, p, p, None) == ARG          # no match starts
    assert L.rrx_group_spans_extents(g._h, 0, p, p, 5, 0, p, None, p, 6, p, p, None) == ARG          # no match ends
    assert L.rrx_group_spans_extents(g._h, 0, p, p, 5, 0, p, p, None, 6, p, p, None) == ARG          # no marks
    assert L.rrx_group_spans_extents(g._h, 0, p, p, 5, 0, p, p, p, 5, p, p, None) == ARG             # marks_words below nitems + 1
    assert b"marks_words" in L.rrx_last_error()
    assert L.rrx_group_spans_extents(g._h, 0, p, p, 5, 0, p, p, p, 6, None, p, None) == ARG          # no group starts
    assert L.rrx_group_spans_extents(g._h, 0, p, p, 5, 0, p, p, p, 6, p, None, None) == ARG          # no group ends
    assert L.rrx_group_spans_extents(bare._h, 0, p, p, 5, 0, None, p, None, 0, p, p, None) == ARG    # marks may be null here, the list may not
    assert L.rrx_group_spans_extents(g._h, 0, None, None, 0, 0, None, None, None, 0, None, None, None) == OK      # an empty batch: nothing to do
    # rrx_extract_group_longest_extents(grp, device, bytes, off, nitems, trim, marks, marks_words, group_start, group_end, stream)
    assert L.rrx_extract_group_longest_extents(None, 0, None, None, 0, 0, None, 0, None, None, None) == ARG
    assert L.rrx_extract_group_longest_extents(g._h, 0, p, None, 5, 0, p, 6, p, p, None) == ARG      # no offsets
    assert L.rrx_extract_group_longest_extents(g._h, 0, p, p, 5, 0, None, 6, p, p, None) == ARG      # no marks
    assert L.rrx_extract_group_longest_extents(g._h, 0, p, p, 5, 0, p, 5, p, p, None) == ARG         # marks_words below nitems + 1
    assert L.rrx_extract_group_longest_extents(g._h, 0, p, p, 5, 0, p, 6, None, p, None) == ARG
    assert L.rrx_extract_group_longest_extents(g._h, 0, p, p, 5, 0, p, 6, p, None, None) == ARG
    assert L.rrx_extract_group_longest_extents(g._h, 0, None, None, 0, 0, None, 0, None, None, None) == OK
    # the items forms
    assert L.rrx_group_spans_items(None, None, None, None, None, 0, None, None, None) == ARG
    assert L.rrx_group_spans_items(g._h, None, p, p, p, 6, p, p, None) == ARG                        # no items handle
    assert L.rrx_extract_group_longest_items(None, None, None, 0, None, None, None) == ARG
    assert L.rrx_extract_group_longest_items(g._h, None, p, 6, p, p, None) == ARG
    assert b"null" in L.rrx_last_error()
    assert L.rrx_group_regex(None) is None and L.rrx_group_program_words(None, 21, None, 0) == 0
