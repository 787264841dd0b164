"""rrx_search_longest_corpus on the CPU: the starts table (kind 19) and the anchored table (kind 20) replayed STRIPE BY STRIPE as
search_longest_corpus_kernel is specified - a lane owns the lines that END in its stripe (from a stripe index modelled from the
text), walks backwards from the end of its stripe with the table at rest behind its last '\\n', follows its first line below the
stripe unless the stripe is fresh, leaves a start and a length per line, then takes its lines forwards on the anchored table up to
the line's '\\n'; a nullable pattern keeps the starts table at rest - against the brute force over the substrings of every line.
The replay issues the kernel's loads (single bytes above the last 16-byte boundary of the data, 128-byte rounds inside the stripe,
16-byte loads below it and in the forward walk) through one function that refuses any byte outside [0, nbytes), and records who
writes which result word: every line has exactly one writer."""
import re

import numpy as np
import pytest

import roaringregex_amd as rr
from contains_cases import split_lines
from program_replay import DfaReplay
from search_longest_corpus_cases import GEOMETRY_PATTERNS, geometry_corpus, geometry_wants, reference_texts

ROUND = 128
NONE = 0xFFFFFFFF


def stripe_index(text, stripe):
    """(base, fresh, nstripes) as the corpus carries them: base[g] = the '\\n' before stripe g (base[nstripes]: all of them), fresh[g]
    = stripe g begins a line."""
    n = len(text)
    nstripes = (n + stripe - 1) // stripe
    nl = np.concatenate([[0], np.cumsum(np.frombuffer(text, dtype=np.uint8) == 10)])
    base = [int(nl[min(g * stripe, n)]) for g in range(nstripes + 1)]
    fresh = [g == 0 or text[g * stripe - 1] == 10 for g in range(nstripes)]
    return base, fresh, nstripes


class CorpusReplay:
    """search_longest_corpus_kernel lane by lane, in Python ints."""

    def __init__(self, r):
        self.nullable = r.accepts_empty
        s, a = r.program(rr.PROGRAM_SEARCH_STARTS), r.program(rr.PROGRAM_SEARCH_ANCHORED)
        assert s is not None and a is not None
        self.s, self.a = DfaReplay(s), DfaReplay(a)
        self.s_cls, self.s_next, self.s_acc = self.s.cls.tolist(), self.s.next.tolist(), self.s.acc.tolist()
        self.a_cls, self.a_next, self.a_acc = self.a.cls.tolist(), self.a.next.tolist(), self.a.acc.tolist()
        assert not self.a_acc[0] and not any(self.a_next[0])
        self.empty = not any(self.a_acc)

    def load(self, at, n, aligned=True):
        """n bytes from offset `at`: inside the data, and a wide load of the backward walk from an aligned offset."""
        assert 0 <= at and at + n <= len(self.text), ("a load outside the data", at, n, len(self.text))
        assert n == 1 or (n in (16, ROUND) and (at % 16 == 0 or not aligned)), (at, n)
        self.loaded += n
        return self.text[at:at + n]

    def store(self, which, line, value, lane):
        assert 0 <= line < self.nlines, ("a word behind the lines", line)
        self.writers[which][line].add(lane)
        self.words[which][line] = value

    def run(self, text, stripe):
        """-> int32 [lines, 2]"""
        self.text, self.nlines, self.loaded = text, len(split_lines(text)), 0
        self.words = [[None] * self.nlines, [None] * self.nlines]
        self.writers = [[set() for _ in range(self.nlines)], [set() for _ in range(self.nlines)]]
        if self.empty:                               # (the entry: two fills, no table, no text)
            return np.full((self.nlines, 2), -1, dtype=np.int32)
        if text:
            self.base, self.fresh, nstripes = stripe_index(text, stripe)
            for g in range(nstripes):
                self.lane(g, stripe, nstripes)
        for which in (0, 1):
            assert all(len(w) == 1 for w in self.writers[which]), "a line without a writer, or with two"
        assert [w for w in self.writers[0]] == [w for w in self.writers[1]]
        out = np.array([self.words[0], self.words[1]], dtype=np.uint32).T.reshape(self.nlines, 2)
        return out.view(np.int32)

    def lane(self, g, stripe, nstripes):
        text, nbytes = self.text, len(self.text)
        b0, b1 = self.base[g], self.base[g + 1]
        fragment = g + 1 == nstripes and text[-1] != 10
        n = b1 - b0 + fragment
        if n <= 0:
            return
        lo = g * stripe
        floor = lo if self.fresh[g] else 0
        st = {"line": n - 1 if fragment else n, "stepping": fragment and not self.nullable, "hit": False, "start": 0, "end": nbytes, "s": self.s.start,
              "first_begin": None}

        def complete(begin):
            length = st["end"] - begin
            self.store(0, b0 + st["line"], 0 if self.nullable else (st["start"] - begin if st["hit"] else NONE), g)
            self.store(1, b0 + st["line"], length, g)
            st["first_begin"] = begin

        def one(c, at):
            if c == 10:
                if st["line"] < 0:
                    return
                if st["line"] < n:
                    complete(at + 1)
                st["line"] -= 1
                st.update(stepping=not self.nullable and st["line"] >= 0, end=at, hit=False, s=self.s.start)
            elif st["stepping"]:
                st["s"] = self.s_next[st["s"]][self.s_cls[c]]
                if self.s_acc[st["s"]]:
                    st.update(hit=True, start=at)

        def down(chunk, at):                         # the bytes of a load, the highest first; a word without '\n' is skipped at rest
            for w in range(len(chunk) - 4, -4, -4):
                if 10 not in chunk[w:w + 4] and not st["stepping"]:
                    continue
                for k in range(3, -1, -1):
                    one(chunk[w + k], at + w + k)

        q = min(lo + stripe, nbytes)
        while q & 15:
            q -= 1
            one(self.load(q, 1)[0], q)
        while q >= lo + ROUND:
            q -= ROUND
            assert st["line"] >= 0
            down(self.load(q, ROUND), q)
        while st["line"] >= 0 and q >= floor + 16:
            q -= 16
            down(self.load(q, 16), q)
        if 0 <= st["line"] < n:
            assert q == floor
            complete(floor)
        assert st["line"] < 0 or (st["line"] == 0 and q == floor)
        # ---- forward, the lane's lines in ascending order
        begin = st["first_begin"]
        for j in range(n):
            length, s = self.words[1][b0 + j], self.words[0][b0 + j]
            assert begin + length == nbytes or text[begin + length] == 10
            e_out = NONE
            if s != NONE:
                e_out = self.longest_end(begin + s, begin + length) - begin
            self.store(1, b0 + j, e_out, g)
            begin += length + 1

    def longest_end(self, start, limit):
        text, nbytes = self.text, len(self.text)
        s, end, a = self.a.start, start, start                 # pieces of 16 bytes counted from the start itself
        while a < limit and s:
            k1 = min(limit - a, 16)
            piece = self.load(a, 16, aligned=False) if a + 16 <= nbytes else None
            for k in range(k1):
                c = piece[k] if piece is not None else self.load(a + k, 1)[0]
                assert c != 10
                s = self.a_next[s][self.a_cls[c]]
                if self.a_acc[s]:
                    end = a + k + 1
                if not s:
                    break
            a += 16
        return end


def check(p, text, want, stripes=(512, 1024), r=None):
    rep = CorpusReplay(r or rr.RRegex(p))
    for stripe in stripes:
        for data in (text, text[:-1]) if len(text) > 1 and text.endswith(b"\n") and not text.endswith(b"\n\n") else (text,):      # ... and without the final '\n'
            got = rep.run(data, stripe)
            assert got.shape == want.shape, (p[:40], stripe, got.shape, want.shape)
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert bad.size == 0, (p[:40], stripe, int(bad[0]), split_lines(data)[bad[0]][:60], got[bad[0]].tolist(), want[bad[0]].tolist())
    return rep


def test_the_replay_against_the_brute_force_on_the_shared_items():
    texts = reference_texts()
    assert len(texts) >= 43
    nullable = stripes = 0
    for p, text, want in texts:
        assert len(text) > 1536 and want.shape == (len(split_lines(text)), 2)
        rep = check(p, text, want)
        nullable += rep.nullable
        stripes += len(rep.base) - 1
        assert rep.loaded >= len(text) - 1 or rep.nullable      # (the starts table never dies: every byte of every line is read)
    assert nullable >= 2 and stripes >= 43


def test_the_corpus_built_by_hand():
    data, _, _ = geometry_corpus()
    wants = geometry_wants()
    for p in GEOMETRY_PATTERNS:
        check(p, data, wants[p], stripes=(512, 1024, 16384))
    # "ab" '\n' "c": a literal and a pattern that holds the '\n' both stay inside their lines
    assert (wants["abc"][9] == -1).all() and (wants["abc"][10] == -1).all() and (wants["a\nb"] == -1).all()


def test_ownership_by_line_end():
    """Who writes what at stripe 512: lane 1 holds no '\\n' and writes nothing, lane 2 owns line 1 whose bytes all lie in stripe 1, lane
    4 owns the 1300-byte line, lane 5 - a fresh stripe - the empty line behind the "\\n\\n"."""
    data, _, _ = geometry_corpus()
    rep = CorpusReplay(rr.RRegex("ab+c"))
    rep.run(data, 512)
    owner = [next(iter(w)) for w in rep.writers[0]]
    assert owner[:9] == [0, 2, 4, 4, 5, 5, 5, 6, 7] and 1 not in owner and 3 not in owner
    assert rep.fresh[1] and rep.fresh[5] and rep.fresh[6] and not rep.fresh[2] and not rep.fresh[4]
    # the final fragment of a text without its last '\n' belongs to the last stripe, which here also ends other lines
    rep.run(data[:-1], 512)
    last = (len(data) - 2) // 512
    assert next(iter(rep.writers[0][-1])) == last and sum(1 for w in rep.writers[0] if last in w) > 1


@pytest.mark.parametrize("text", [b"", b"\n", b"a", b"aab\n\nb", b"\n" * 600, b"z" * 700, b"z" * 505 + b"aaa\naaaa" + b"z" * 600 + b"\naa"])
def test_nullable_empty_language_and_the_ends_of_the_data(text):
    lines = split_lines(text)
    want = np.array([(0, len(ln) - len(ln.lstrip(b"a"))) for ln in lines], dtype=np.int32).reshape(len(lines), 2)
    check("a*", text, want)
    check("[]", text, np.full((len(lines), 2), -1, dtype=np.int32))
    runs = [m.span() if m else (-1, -1) for m in (re.search(rb"a+", ln) for ln in lines)]
    check("a+", text, np.array(runs, dtype=np.int32).reshape(len(lines), 2))
