"""regexp_extract_all / split from a match list (rrx_pieces_sizes / _fill, rrx_extract_all_longest_*, rrx_split_longest_*) on the
CPU: both kernels of kernels_pieces_items.hip replayed in Python ints AS THEY ARE SPECIFIED - pieces_sizes_kernel a lane per item
(the list offsets, the clamped pieces as (source offset, length)), pieces_fill_kernel driven by output bytes: the chunks cut at
dword-aligned addresses and handed out grid-stride, the two 64-way searches of a chunk, per dword the lane's own search and the piece
carried from byte to byte, the wide loads; every store checked for "once, inside the range, aligned" and every load for "inside the
piece" - against THE RULE (matches: t[s_k:e_k]; gaps: t[e_{k-1}:s_k]) on every (pattern, items, lists) of
test_search_all_longest_items_lowering's reference_all(), against re.findall / re.split where Python's greedy search names the same
lists, on the named cases of include/rrx.h and on lists that are not the items'.  Also the entries' argument checks, which need no
device."""
import bisect
import random
import re

import numpy as np

import roaringregex_amd as rr
from contains_cases import EXPLODING
from test_contains_items_lowering import MAX_ITEM
from test_replace_items_lowering import csr_lists, span, splice
from test_search_all_longest_items_lowering import GREEDY_ALL_RE, SEED, finditer_all, pack, reference_all, want_for

POISON = 0x5A
MARGIN = 64
CHUNK = 4096                                        # device.hpp: kPiecesChunk
M64 = (1 << 64) - 1


def clamp(x, lo, hi):
    return lo if x < lo else hi if x > hi else x


def pieces_rule(item, matches, gaps):
    """The rule with its clamping: the pieces of one item as bytes.  For a list of the item's own the clamps are the identity."""
    out, a, L = [], 0, len(item)
    for s, e in matches:
        s = clamp(s, a, L)
        e = clamp(e, s, L)
        out.append(item[a:s] if gaps else item[s:e])
        a = e
    if gaps:
        out.append(item[a:])
    return out


def sizes_replay(offs, trim, first, start, end, gaps):
    """pieces_sizes_kernel: a lane per item -> (list_off[n + 1], piece_len by slot, piece_src by slot); every slot stored once."""
    n = len(offs) - 1
    npieces = first[n] - first[0] + (n if gaps else 0)
    list_off, length, src = [None] * (n + 1), [None] * npieces, [None] * npieces
    for i in range(n):
        b, e = span(offs, i, trim)
        L, base, f0, f1 = e - b, first[0], first[i], first[i + 1]
        slot = f0 - base + (i if gaps else 0)
        list_off[i] = slot
        if i + 1 == n:
            list_off[n] = f1 - base + (n if gaps else 0)

        def piece(lo, hi):
            nonlocal slot
            assert 0 <= lo <= hi <= L and length[slot] is None
            src[slot] = b + lo
            length[slot] = min(hi - lo, 0xffffffff)
            slot += 1

        a = 0
        for k in range(f0, f1):
            s = clamp(start[k], a, L)
            en = clamp(end[k], s, L)
            piece(a, s) if gaps else piece(s, en)
            a = en
        if gaps:
            piece(a, L)
    assert None not in list_off and None not in length and None not in src, "exactly the slots 0 .. npieces - 1 and the n + 1 list words"
    return list_off, length, src


class Rounds:
    n = 0


def wave_last_le(v, a, b, q, rounds=None):
    """The 64-way search: the last index in [a, b) with v[idx] <= q (v ascending, v[a] <= q); lane l probes a + l * step."""
    while b - a > 1:
        step = (b - a + 63) >> 6
        votes = [a + lane * step < b and v[a + lane * step] <= q for lane in range(64)]
        k = sum(votes)
        assert votes[0] and votes == [True] * k + [False] * (64 - k), "a prefix of the lanes, lane 0 among them"
        a += (k - 1) * step
        b = min(a + step, b)
        if rounds is not None:
            rounds.n += 1
    return a


class FillReplay:
    """pieces_fill_kernel: `out` is a bytearray standing at address out_addr, the byte buffer at bytes_addr (their residues mod 4
    matter); `waves` = the waves of the grid, `chunk` = kPiecesChunk (the replay takes any multiple of 4: the small reference
    batches are cut into many chunks that way)."""

    def __init__(self, text, src, off, out, out_addr=0, bytes_addr=0, chunk=CHUNK, waves=8):
        assert chunk % 4 == 0
        self.text, self.src, self.off, self.npieces = text, src, off, len(off) - 1
        self.out, self.out_addr, self.bytes_addr, self.chunk, self.waves = out, out_addr, bytes_addr, chunk, waves
        self.written = bytearray(len(out))
        self.dword_stores = self.byte_stores = self.locates = self.steps = self.chunks = self.rounds = self.far = 0
        self.loads = {1: 0, 4: 0, 8: 0}

    def store(self, at, value, width):
        assert 0 <= at and at + width <= len(self.out)
        for k in range(width):
            assert not self.written[at + k], ("a byte stored twice", at + k)
            self.written[at + k] = 1
            self.out[at + k] = (value >> (8 * k)) & 0xff

    def load(self, at, width, p):
        """`width` bytes of the byte buffer at offset `at`, all of them inside piece p, an aligned load if it is a wide one."""
        assert self.src[p] <= at and at + width <= self.src[p] + self.off[p + 1] - self.off[p], ("a byte outside the piece is read", p, at, width)
        assert width == 1 or (self.bytes_addr + at) % 4 == 0
        return sum(self.text[at + k] << (8 * k) for k in range(width))

    def run(self):
        if not self.npieces:
            return
        off, n = self.off, self.npieces
        lo, hi = off[0], off[n]
        if hi <= lo:
            return
        mis = (self.out_addr + lo) & 3
        total = hi - lo + mis
        nchunks = (total + self.chunk - 1) // self.chunk
        for wave in range(self.waves):
            for c in range(wave, nchunks, self.waves):
                self.one_chunk(c, lo, hi, mis, total)

    def one_chunk(self, c, lo, hi, mis, total):
        off, src, n = self.off, self.src, self.npieces
        self.chunks += 1
        rel0 = c * self.chunk
        rel1 = min(rel0 + self.chunk, total)
        q_first, q_last = lo + (0 if rel0 < mis else rel0 - mis), lo + rel1 - mis - 1
        assert lo <= q_first <= q_last < hi
        r = Rounds()
        pa = wave_last_le(off, 0, n, q_first, r)
        near = pa + self.chunk + 1
        if near < n and off[near] <= q_last:
            self.far += 1                                           # more pieces begin inside the chunk than it has bytes: empty ones
        if near >= n or off[near] <= q_last:
            near = n
        pb = wave_last_le(off, pa, near, q_last, r)
        self.rounds += r.n
        assert pa == bisect.bisect_right(off, q_first, 0, n) - 1 and pb == bisect.bisect_right(off, q_last, 0, n) - 1
        for rel in range(rel0, rel1, 4):                            # (lane = rel / 4 % 64, turn = rel / 256 % 16)
            c0 = mis - rel if rel < mis else 0
            c1 = min(total - rel, 4)
            assert c0 < c1
            state = {"p": pa}

            def locate(q):
                self.locates += 1
                p, above = state["p"], pb
                while p < above:
                    self.steps += 1
                    mid = p + ((above - p + 1) >> 1)
                    if off[mid] <= q:
                        p = mid
                    else:
                        above = mid - 1
                assert off[p] <= q < off[p + 1]
                state["p"] = p
                return p, off[p + 1], (src[p] - off[p]) & M64

            q0 = lo + rel + c0 - mis
            p, lim, origin = locate(q0)
            at = (origin + q0) & M64
            word = 0
            if c0 == 0 and c1 == 4 and lim - q0 >= 4:
                sh = (self.bytes_addr + at) & 3
                if sh == 0:
                    self.loads[4] += 1
                    word = self.load(at, 4, p)
                elif q0 - off[p] >= sh and lim - q0 >= 8 - sh:
                    self.loads[8] += 1
                    word = ((self.load(at - sh, 4, p) | self.load(at - sh + 4, 4, p) << 32) >> (8 * sh)) & 0xffffffff
                else:
                    self.loads[1] += 4
                    word = sum(self.load(at + k, 1, p) << (8 * k) for k in range(4))
            else:
                for cc in range(c0, c1):
                    q = q0 + cc - c0
                    if q >= lim:
                        p, lim, origin = locate(q)
                    self.loads[1] += 1
                    word |= self.load((origin + q) & M64, 1, p) << (8 * cc)
            dst = lo + rel - mis                                    # an offset into out; out_addr + dst is 4-byte aligned
            assert (self.out_addr + dst) % 4 == 0
            if c0 == 0 and c1 == 4:
                self.dword_stores += 1
                self.store(dst, word, 4)
            else:
                for cc in range(c0, c1):
                    self.byte_stores += 1
                    self.store(dst + cc, (word >> (8 * cc)) & 0xff, 1)


def fill_checked(text, src, piece_off, **kw):
    """FillReplay on poisoned output: exactly [piece_off[0], piece_off[n]) is written -> (out, the replay)."""
    lo, hi = piece_off[0], piece_off[-1]
    out = bytearray([POISON]) * (hi + MARGIN)
    f = FillReplay(text, src, piece_off, out, **kw)
    f.run()
    assert all(f.written[lo:hi]) and not any(f.written[:lo]) and not any(f.written[hi:]), "exactly [piece_off[0], piece_off[npieces])"
    assert bytes(out[:lo]) == bytes([POISON]) * lo and bytes(out[hi:]) == bytes([POISON]) * MARGIN
    return out, f


def replay(items, lists, gaps, trim=0, lead=0, out_first=0, out_addr=0, bytes_addr=0, first0=0, chunk=CHUNK, waves=8):
    """One batch through both kernels -> (the pieces per item, the FillReplay for its counters).  out_first: d_piece_off[0], a
    running offset into a larger buffer; first0: the batch's first slot, d_first[0]."""
    text, offs = pack(items, trim, lead, seed=len(items))
    text = text.tolist()
    n = len(items)
    first, start, end = csr_lists(lists, first0)
    list_off, length, src = sizes_replay(offs, trim, first, start, end, gaps)
    assert list_off[0] == 0 and list_off[n] == len(length)
    assert list_off == [first[i] - first0 + (i if gaps else 0) for i in range(n + 1)]
    piece_off = [out_first]
    for x in length:
        piece_off.append(piece_off[-1] + x)
    out, f = fill_checked(text, src, piece_off, out_addr=out_addr, bytes_addr=bytes_addr, chunk=chunk, waves=waves)
    pieces = [bytes(out[piece_off[p]:piece_off[p + 1]]) for p in range(len(length))]
    return [pieces[list_off[i]:list_off[i + 1]] for i in range(n)], f


def check(items, lists, gaps, **kw):
    got, f = replay(list(items), lists, gaps, **kw)
    for k, (g, it, w) in enumerate(zip(got, items, lists)):
        assert g == pieces_rule(it, w, gaps), (k, it, w, gaps, g)
    return got, f


def test_replay_against_the_rule():
    dwords = singles = out_bytes = chunks = wide = 0
    for n_p, (p, items, want) in enumerate(reference_all()):
        for trim, lead in ((0, 5), (1, 37)):
            # the output buffer and the byte buffer at every residue mod 4, d_piece_off[0] and d_first[0] not 0; the kernel's chunk (one
            # chunk holds such a batch) and a chunk of 64 bytes (dozens of them, taken grid-stride by five waves)
            for chunk, waves in ((CHUNK, 8), (64, 5)):
                kw = dict(trim=trim, lead=lead, out_first=(n_p + trim) % 7 + 1, out_addr=(n_p + trim + chunk) % 4, bytes_addr=(n_p // 4 + trim) % 4,
                          first0=n_p % 3 + 1, chunk=chunk, waves=waves)
                matches, f = check(items, want, False, **kw)
                gaps, g = check(items, want, True, **kw)
                for it, m, gp, w in zip(items, matches, gaps, want):
                    assert len(m) == len(w) and len(gp) == len(w) + 1
                    assert sum(map(len, m)) + sum(map(len, gp)) == len(it)
                    assert b"".join(gp) == splice(it, w, b"")
                    assert m == [it[s:e] for s, e in w] and b"".join(x + y for x, y in zip(gp, m + [b""])) == it
                for r in (f, g):
                    dwords += r.dword_stores
                    singles += r.byte_stores
                    chunks += r.chunks
                    wide += r.loads[4] + r.loads[8]
                out_bytes += sum(len(x) for m in matches for x in m) + sum(len(x) for gp in gaps for x in gp)
    # d_out at every residue mod 4 for ONE batch (every fifth pattern), the byte buffer at another one each time
    for n_p, (p, items, want) in enumerate(reference_all()[::5]):
        for out_addr in range(4):
            for gaps in (False, True):
                check(items, want, gaps, trim=n_p % 2, lead=3, out_first=n_p % 5, out_addr=out_addr, bytes_addr=(out_addr + 1 + n_p) % 4, first0=2,
                      chunk=(CHUNK, 64)[out_addr % 2], waves=3)
    print("output bytes", out_bytes, "dword stores", dwords, "byte stores", singles, "chunks", chunks, "wide loads", wide)
    assert out_bytes == 4 * dwords + singles
    assert 0 < singles <= 6 * 4 * 2 * len(reference_all()), "byte stores only at the partial first and last dwords of a whole range"
    assert chunks > 20 * len(reference_all()) and wide > 0


def test_against_findall_and_split():
    """Where Python's greedy search names the leftmost-longest list (test_search_all_longest_items_lowering checks that), the replay on
    re.finditer's list is re.findall and re.split; on short items the list is the oracle's brute force."""
    rng = random.Random(SEED + 31)
    for p, rx in GREEDY_ALL_RE.items():
        alphabet = "01 29a" if p == "[0-9]+" else "aabbc z"
        items = ["".join(rng.choice(alphabet) for _ in range(rng.randrange(MAX_ITEM + 1))).encode() for _ in range(150)]
        lists = want_for(p, items)
        assert lists == [finditer_all(p, it) for it in items]
        items += ["".join(rng.choice(alphabet) for _ in range(rng.randrange(200, 700))).encode() for _ in range(20)] + [b""]
        lists = [finditer_all(p, it) for it in items]
        assert sum(len(w) >= 2 for w in lists) >= 20
        for chunk in (CHUNK, 256):
            got, _ = replay(items, lists, False, trim=1, lead=3, out_first=5, out_addr=chunk % 3, bytes_addr=1, chunk=chunk)
            assert got == [re.findall(rx, it) for it in items], p
            got, _ = replay(items, lists, True, trim=1, lead=3, out_first=5, out_addr=3, bytes_addr=2, chunk=chunk)
            assert got == [re.split(rx, it) for it in items], p
    # a pattern that accepts the empty string: Python >= 3.7 and the brute force name the same list
    items = [b"baab", b"", b"aa", b"bbb", b"aabaa" * 20]
    lists = [[(m.start(), m.end()) for m in re.finditer(rb"a*", it)] for it in items]
    assert want_for("a*", items[:4]) == lists[:4]
    assert replay(items, lists, False, trim=1)[0] == [re.findall(rb"a*", it) for it in items]
    assert replay(items, lists, True, trim=1, chunk=16)[0] == [re.split(rb"a*", it) for it in items]


def test_named_cases():
    for p, item, matches, gaps in (("[0-9]+", b"a1 22 333", [b"1", b"22", b"333"], [b"a", b" ", b" ", b""]),
                                   ("a*", b"baab", [b"", b"aa", b"", b""], [b"", b"b", b"", b"b", b""])):
        lists = want_for(p, [item])
        assert check([item], lists, False)[0] == [matches] and check([item], lists, True)[0] == [gaps]
        batch, blists = [b"", item, b"", item], [want_for(p, [b""])[0], lists[0], want_for(p, [b""])[0], lists[0]]
        for gaps_mode, want in ((False, matches), (True, gaps)):
            got, _ = check(batch, blists, gaps_mode, trim=1, lead=31, out_first=3, out_addr=1, bytes_addr=3, chunk=8)
            assert got[1] == got[3] == want
    # items without matches: extract gives empty lists and writes nothing, split gives the items - the separators never copied
    items = [b"x" * (k % 7) for k in range(130)]
    got, f = check(items, [[] for _ in items], False, trim=3, lead=2)
    assert got == [[] for _ in items] and f.chunks == 0
    got, f = check(items, [[] for _ in items], True, trim=3, lead=2, out_first=1, out_addr=2, chunk=64)
    assert got == [[it] for it in items]
    # everything matched: the gaps are all empty - pieces, and not a byte
    got, f = check([b"abc"] * 70, [[(0, 3)]] * 70, True, trim=1)
    assert got == [[b"", b""]] * 70 and f.chunks == 0
    # a*  on b's through MATCHES: runs of 65 and of 5000 empty pieces astride a chunk's first byte ("the last p with offset <= q" skips them)
    for run in (65, 5000):
        items = [b"a" * 4095, b"b" * (run - 2), b"aaaaaaa"]
        lists = [[(m.start(), m.end()) for m in re.finditer(rb"a*", it)] for it in items]
        assert sum(len(w) for w in lists) == 2 + (run - 1) + 2 and lists[1] == [(k, k) for k in range(run - 1)]
        got, f = check(items, lists, False, out_first=1)
        assert got == [re.findall(rb"a*", it) for it in items] and f.chunks == 2 and f.far == 0       # (pa already sits behind the run)
    # the run of 5000 strictly INSIDE a chunk: more pieces begin in the chunk than the kPiecesChunk + 1 entries behind pa hold, so the
    # search for pb takes the whole rest of the offsets (`near = npieces`); a run of 65 there stays within the near entries
    for run, far in ((65, 0), (5000, 1)):
        items = [b"a" * 100, b"b" * (run - 2), b"aaaaaaa"]
        lists = [[(m.start(), m.end()) for m in re.finditer(rb"a*", it)] for it in items]
        for out_addr in (0, 3):
            got, f = check(items, lists, False, out_first=2, out_addr=out_addr)
            assert got == [re.findall(rb"a*", it) for it in items] and f.chunks == 1 and f.far == far, (run, f.far)


def test_the_64_way_search():
    """wave_last_le against bisect on ascending arrays with runs of equal entries, up to 300000 entries: the rounds it takes."""
    rng = random.Random(SEED + 32)
    for n in (1, 2, 63, 64, 65, 4096, 4097, 300000):
        v, at = [], 10
        for _ in range(n + 1):
            v.append(at)
            at += rng.choice((0, 0, 1, 3, 40))
        for q in [v[0], v[-1] - 1 if v[-1] > v[0] else v[0], v[n // 2]] + [rng.randrange(v[0], max(v[-1], v[0] + 1)) for _ in range(20)]:
            r = Rounds()
            assert wave_last_le(v, 0, n, q, r) == bisect.bisect_right(v, q, 0, n) - 1
            rounds = 0
            while 64 ** rounds < n:
                rounds += 1
            assert r.n <= rounds, (n, r.n)


def test_lists_that_are_not_the_items_come_out_clamped():
    rng = random.Random(SEED + 33)
    items = [bytes(rng.choice(b"abc") for _ in range(rng.randrange(12))) for _ in range(100)]
    # starts and ends beyond the item, unordered, e < s
    lists = [[(rng.randrange(40), rng.randrange(40)) for _ in range(rng.randrange(4))] for _ in items]
    assert any(e < s for w in lists for s, e in w) and any(s > len(it) for it, w in zip(items, lists) for s, e in w)
    assert any(len(w) > 1 and w[1][0] < w[0][1] for w in lists)
    for gaps in (False, True):
        got, _ = check(items, lists, gaps, trim=1, lead=3, out_first=2, out_addr=3, bytes_addr=1, chunk=32)
        for it, pieces in zip(items, got):
            assert len(b"".join(pieces)) <= len(it)
    assert pieces_rule(b"abcdef", [(4, 2), (1, 3), (9, 12), (0xffffffff, 0xffffffff)], True) == [b"abcd", b"", b"ef", b"", b""]
    assert pieces_rule(b"abcdef", [(4, 2), (1, 5), (9, 12)], False) == [b"", b"e", b""]
    # sizes: a piece beyond 32 bits saturates (one item of 5 GB without a match, split)
    offs = np.array([0, 5 << 30, (5 << 30) + 4], dtype=np.int64)
    list_off, length, src = sizes_replay(offs, 0, [7, 7, 8], [None] * 7 + [1], [None] * 7 + [3], True)
    assert list_off == [0, 1, 3] and length == [0xffffffff, 1, 1] and src == [0, 5 << 30, (5 << 30) + 3]
    # fill takes any ascending offsets and any sources: every byte of the range once, nothing else
    text = list(range(256)) * 4
    piece_off, src = [3], []
    for _ in range(300):
        n = rng.choice((0, 0, 1, 2, 5, 9, 40))
        src.append(rng.randrange(len(text) - n))
        piece_off.append(piece_off[-1] + n)
    for out_addr in range(4):
        out, _ = fill_checked(text, src, piece_off, out_addr=out_addr, bytes_addr=out_addr ^ 1, chunk=128, waves=3)
        assert all(bytes(out[piece_off[p]:piece_off[p + 1]]) == bytes(text[src[p]:src[p] + piece_off[p + 1] - piece_off[p]]) for p in range(300))


def test_arguments_are_checked_without_a_device():
    r = rr.RRegex("ab+c")
    L, C = rr._L, rr.C
    p = C.cast((C.c_uint64 * 8)(), C.c_void_p)
    npc, tot = C.byref(C.c_size_t(0)), C.byref(C.c_size_t(0))
    ARG, UNSUPPORTED = 2, 4
    assert (rr.PIECES_MATCHES, rr.PIECES_GAPS) == (0, 1)
    # rrx_pieces_sizes(device, off, nitems, trim, first, start, end, mode, list_off, piece_len, piece_src, stream)
    ok = [0, p, 5, 0, p, p, p, 1, p, p, p, None]
    for k in (1, 4, 5, 6, 8, 9, 10):
        a = list(ok)
        a[k] = None
        assert L.rrx_pieces_sizes(*a) == ARG, k
        assert b"null" in L.rrx_last_error()
    for mode in (2, -1):
        a = list(ok)
        a[7] = mode
        assert L.rrx_pieces_sizes(*a) == ARG and b"mode" in L.rrx_last_error()
        assert L.rrx_pieces_sizes(0, None, 0, 0, None, None, None, mode, None, None, None, None) == ARG
    for mode in (0, 1):
        assert L.rrx_pieces_sizes(0, None, 0, 0, None, None, None, mode, None, None, None, None) == 0          # nitems == 0: nothing to do
    # rrx_pieces_fill(device, bytes, piece_src, piece_off, npieces, out, stream)
    ok = [0, p, p, p, 5, p, None]
    for k in (2, 3):
        a = list(ok)
        a[k] = None
        assert L.rrx_pieces_fill(*a) == ARG, k
    assert L.rrx_pieces_fill(0, None, None, None, 0, None, None) == 0
    # rrx_*_longest_extents(re, device, bytes, off, nitems, trim, list_off, piece_off, pieces_cap, out, cap, npieces, total, stream)
    bad = rr.RRegex(EXPLODING)
    assert bad.program(rr.PROGRAM_SEARCH_STARTS) is None
    for extents, items in ((L.rrx_extract_all_longest_extents, L.rrx_extract_all_longest_items), (L.rrx_split_longest_extents, L.rrx_split_longest_items)):
        ok = [r._h, 0, p, p, 5, 0, p, p, 9, p, 9, npc, tot, None]
        for k in (0, 3, 6, 7, 9, 11, 12):
            a = list(ok)
            a[k] = None
            assert extents(*a) == ARG, k
            assert b"null" in L.rrx_last_error()
        assert extents(r._h, 0, None, None, 0, 0, None, p, 0, None, 0, npc, tot, None) == ARG           # no d_list_off, for an empty batch too
        assert extents(r._h, 0, None, None, 0, 0, p, None, 0, None, 0, npc, tot, None) == ARG           # no d_piece_off
        # rrx_*_longest_items(re, items, list_off, piece_off, pieces_cap, out, cap, npieces, total, stream)
        assert items(None, None, p, p, 9, p, 9, npc, tot, None) == ARG
        assert items(r._h, None, p, p, 9, p, 9, npc, tot, None) == ARG                                   # no items handle
        assert b"null" in L.rrx_last_error()
        # a regex without leftmost-longest tables is reported for an empty batch, without a device
        assert extents(bad._h, 0, None, None, 0, 0, p, p, 0, None, 0, npc, tot, None) == UNSUPPORTED
        assert b"determinise" in L.rrx_last_error()
