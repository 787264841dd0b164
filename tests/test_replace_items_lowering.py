"""regexp_replace from a match list (rrx_replace_matches_sizes / _fill, rrx_replace_all_longest_*) on the CPU: both kernels of
kernels_replace_items.hip replayed in Python ints AS THEY ARE SPECIFIED - replace_sizes_kernel a lane per item (d_len, d_pos),
replace_fill_kernel a wave per 64 items driven by output bytes: the 64 staged output offsets, the sweep in dwords aligned by
address, per byte the item search, the d_pos search and the source, the segment carried from byte to byte - against the SPLICE RULE
t[0:s_0] + R + t[e_0:s_1] + ... + R + t[e_{m-1}:] on every (pattern, items, lists) of test_search_all_longest_items_lowering's
reference_all(), against re.sub where Python's greedy search names the same lists, and on the named cases of include/rrx.h.  Also
the entries' argument checks, which need no device."""
import random
import re

import numpy as np

import roaringregex_amd as rr
from contains_cases import EXPLODING
from test_contains_items_lowering import MAX_ITEM, oracle_for
from test_search_all_items_lowering import all_brute_force as lazy_all_brute_force
from test_search_all_longest_items_lowering import GREEDY_ALL_RE, SEED, finditer_all, pack, reference_all, want_for

POISON = 0x5A
MARGIN = 64
REPLACEMENTS = (b"", b"X", b"<<>>", bytes(range(33, 133)))         # 0, 1, 4 and 100 bytes: the last one longer than a lane's dword and than most items
M64 = (1 << 64) - 1


def splice(item, matches, rep):
    """The rule: the item with every match of the list replaced by `rep`."""
    out, at = [], 0
    for s, e in matches:
        assert at <= s <= e <= len(item)
        out.append(item[at:s])
        out.append(rep)
        at = e
    out.append(item[at:])
    return b"".join(out)


def csr_lists(lists, first0=0):
    """[[(s, e)]] per item -> (first[n + 1], start, end); the slots begin at first0: the arrays are indexed by the slot itself."""
    first, start, end = [first0], [None] * first0, [None] * first0
    for w in lists:
        for s, e in w:
            start.append(s)
            end.append(e)
        first.append(len(start))
    return first, start, end


def span(offs, i, trim):
    b, e = int(offs[i]), int(offs[i + 1])
    return b, (e - trim if e - b >= trim else b)


def sizes_replay(offs, trim, first, start, end, rep_len):
    """replace_sizes_kernel: a lane per item -> (d_len[n], d_pos by slot; None where the kernel stores nothing)."""
    n = len(offs) - 1
    length, pos = [], [None] * len(start)
    for i in range(n):
        b, e = span(offs, i, trim)
        shift = 0                                                   # (k * rep_len - removed) mod 2^64
        for slot in range(first[i], first[i + 1]):
            assert pos[slot] is None
            pos[slot] = (start[slot] + shift) & 0xffffffff
            shift = (shift + rep_len - (end[slot] - start[slot])) & M64
        total = (e - b + shift) & M64
        if total >> 63:
            total = 0
        length.append(min(total, 0xffffffff))
    return length, pos


class FillReplay:
    """replace_fill_kernel on a batch: out is a bytearray standing at address `out_addr` (only its residue mod 4 matters)."""

    def __init__(self, text, offs, trim, first, end, pos, rep, out_off, out, out_addr):
        self.text, self.offs, self.trim, self.first, self.end, self.pos, self.rep = text, offs, trim, first, end, pos, rep
        self.out_off, self.out, self.out_addr = out_off, out, out_addr
        self.written = bytearray(len(out))
        self.dword_stores = self.byte_stores = self.locates = self.pos_steps = self.passes = 0

    def store(self, at, value, width):
        assert 0 <= at and at + width <= len(self.out)
        for k in range(width):
            assert not self.written[at + k], ("a byte stored twice", at + k)
            self.written[at + k] = 1
            self.out[at + k] = (value >> (8 * k)) & 0xff

    def run(self):
        n = len(self.offs) - 1
        for first_item in range(0, n, 64):
            self.wave_pass(first_item, n)

    def wave_pass(self, F, n):
        row = [self.out_off[min(F + lane, n)] for lane in range(64)] + [self.out_off[min(F + 64, n)]]
        lo, hi = row[0], row[64]
        if hi <= lo:
            return
        self.passes += 1
        mis = (self.out_addr + lo) & 3
        total = hi - lo + mis
        pos, first, rep_len = self.pos, self.first, len(self.rep)
        for rel in range(0, total, 4):                              # (lane = rel / 4 % 64, turn = rel / 256)
            c0 = mis - rel if rel < mis else 0
            c1 = min(total - rel, 4)
            assert c0 < c1
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
                        self.pos_steps += 1
                        mid = below + ((above - below) >> 1)
                        if pos[mid] <= r:
                            below = mid + 1
                        else:
                            above = mid
                    lim = o1
                    if below < f1:
                        lim = min(lim, o0 + pos[below])
                    in_rep, origin = False, o0
                    if below > f0:
                        at = o0 + pos[below - 1]
                        if q - at < rep_len:
                            in_rep, origin, lim = True, at, min(lim, at + rep_len)
                        else:
                            origin = at + rep_len - self.end[below - 1]
                    assert lim > q
                src = (q - origin) & M64
                v = self.rep[src] if in_rep else (self.text[b + src] if src < item_len else 0)
                word |= v << (8 * c)
            dst = lo + rel - mis                                    # an offset into out; out_addr + dst is 4-byte aligned
            assert (self.out_addr + dst) % 4 == 0
            if c0 == 0 and c1 == 4:
                self.dword_stores += 1
                self.store(dst, word, 4)
            else:
                for c in range(c0, c1):
                    self.byte_stores += 1
                    self.store(dst + c, (word >> (8 * c)) & 0xff, 1)


def replay(items, lists, rep, trim=0, lead=0, out_first=0, out_addr=0, first0=0):
    """One batch through both kernels -> (the output items, the FillReplay for its counters).  out_first: d_out_off[0], a running
    offset into a larger buffer; first0: the batch's first slot, d_first[0]."""
    text, offs = pack(items, trim, lead, seed=len(items))
    text = text.tolist()
    n = len(items)
    first, start, end = csr_lists(lists, first0)
    length, pos = sizes_replay(offs, trim, first, start, end, len(rep))
    assert len(length) == n
    assert all((p is None) == (slot < first0) for slot, p in enumerate(pos)), "exactly the slots first[0] .. first[n] are stored"
    out_off = [out_first]
    for x in length:
        out_off.append(out_off[-1] + x)
    out = bytearray([POISON]) * (out_off[-1] + MARGIN)
    f = FillReplay(text, offs, trim, first, end, pos, rep, out_off, out, out_addr)
    f.run()
    assert all(f.written[out_first:out_off[-1]]) and not any(f.written[:out_first]) and not any(f.written[out_off[-1]:]), "exactly [out_off[0], out_off[n])"
    assert bytes(out[:out_first]) == bytes([POISON]) * out_first and bytes(out[out_off[-1]:]) == bytes([POISON]) * MARGIN
    return [bytes(out[out_off[i]:out_off[i + 1]]) for i in range(n)], f


def check(items, lists, rep, **kw):
    got, f = replay(list(items), lists, rep, **kw)
    for k, (g, it, w) in enumerate(zip(got, items, lists)):
        assert g == splice(it, w, rep), (k, it, w, rep[:8], g)
    return got, f


def test_replay_against_the_splice_rule():
    dwords = singles = locates = steps = out_bytes = passes = 0
    for n_p, (p, items, want) in enumerate(reference_all()):
        for n_r, rep in enumerate(REPLACEMENTS):
            for trim, lead in ((0, 5), (1, 37)):
                # the output buffer at every residue mod 4, d_out_off[0] and d_first[0] not 0
                got, f = check(items, want, rep, trim=trim, lead=lead, out_first=(n_p + trim) % 7, out_addr=(n_p + n_r + trim) % 4, first0=n_p % 3)
                dwords += f.dword_stores
                singles += f.byte_stores
                locates += f.locates
                steps += f.pos_steps
                out_bytes += sum(len(g) for g in got)
                passes += f.passes
    print("output bytes", out_bytes, "dword stores", dwords, "byte stores", singles, "locates", locates, "pos steps", steps)
    assert out_bytes == 4 * dwords + singles
    assert 0 < singles <= 6 * passes, "byte stores only at the passes' partial first and last dwords"
    assert out_bytes // 4 <= locates < out_bytes and steps > 0      # (at least one per dword: the segment is carried inside a lane's dword only)


def test_against_re_sub():
    """Where Python's greedy search names the leftmost-longest list (test_search_all_longest_items_lowering checks that), the replay
    on re.finditer's list is re.sub with a literal replacement; on short items the list is the oracle's brute force."""
    rng = random.Random(SEED + 21)
    for p, rx in GREEDY_ALL_RE.items():
        alphabet = "01 29a" if p == "[0-9]+" else "aabbc z"
        items = ["".join(rng.choice(alphabet) for _ in range(rng.randrange(MAX_ITEM + 1))).encode() for _ in range(150)]
        lists = want_for(p, items)
        assert lists == [finditer_all(p, it) for it in items]
        items += ["".join(rng.choice(alphabet) for _ in range(rng.randrange(200, 700))).encode() for _ in range(20)] + [b""]
        lists = [finditer_all(p, it) for it in items]
        assert sum(len(w) >= 2 for w in lists) > 20
        for rep in REPLACEMENTS:
            got, _ = replay(items, lists, rep, trim=1, lead=3, out_first=5, out_addr=len(rep) % 4)
            assert got == [re.sub(rx, lambda m: rep, it) for it in items], (p, rep[:8])
    # a pattern that accepts the empty string: Python >= 3.7 and the brute force name the same list
    items = [b"baab", b"", b"aa", b"bbb", b"aabaa" * 20]
    lists = [[(m.start(), m.end()) for m in re.finditer(rb"a*", it)] for it in items]
    assert want_for("a*", items[:4]) == lists[:4]
    for rep in REPLACEMENTS:
        got, _ = replay(items, lists, rep, trim=1)
        assert got == [re.sub(rb"a*", lambda m: rep, it) for it in items]


def test_named_cases():
    for p, item, want in (("a*", b"baab", b"<>b<><>b<>"), ("[0-9]+", b"a1 22 333", b"a<> <> <>"), ("ab|b+", b"abbbab", b"<><><>")):
        lists = want_for(p, [item])
        got, _ = check([item], lists, b"<>")
        assert got == [want], (p, item, got)
        got, _ = check([b"", item, b"", item], [want_for(p, [b""])[0], lists[0], want_for(p, [b""])[0], lists[0]], b"<>", trim=1, lead=31, out_first=3, out_addr=1)
        assert got[1] == got[3] == want
    # matches side by side with nothing between them, and one at either end of the item
    assert want_for("ab|b+", [b"abbbab"]) == [[(0, 2), (2, 4), (4, 6)]]
    item, adjacent = b"a1 22 333", lazy_all_brute_force(oracle_for("[0-9]+"), b"a1 22 333")
    assert adjacent == [(1, 2), (3, 4), (4, 5), (6, 7), (7, 8), (8, 9)]       # rrx_search_all_extents' list: the generic entries take it as well
    for rep, want in ((b"<>", b"a<> <><> <><><>"), (b"", b"a  "), (b"#", b"a# ## ###")):
        assert check([item, item], [adjacent, adjacent], rep, trim=1)[0] == [want, want]
    # an item without matches is copied verbatim, the separators never: 130 items = three passes of a wave, the middle one partial dwords on both sides
    items = [b"x" * (k % 7) for k in range(130)]
    got, f = check(items, [[] for _ in items], b"R", trim=3, lead=2, out_first=1, out_addr=2)
    assert got == items and f.pos_steps == 0
    # everything matched and R empty: nothing to write
    got, f = check([b"abc"] * 70, [[(0, 3)]] * 70, b"", trim=1)
    assert got == [b""] * 70 and f.locates == 0


def test_lengths_saturate_and_lists_that_are_not_the_items_do_no_harm():
    # sizes: a length beyond 32 bits saturates (one item of 5 GB and a replacement that grows it), a list that removes more than the item holds gives 0
    offs = np.array([0, 5 << 30, (5 << 30) + 4], dtype=np.int64)
    length, pos = sizes_replay(offs, 0, [0, 1, 2], [3, 0], [4, 9], 7)
    assert length == [0xffffffff, 2] and pos == [3, 0]
    length, pos = sizes_replay(offs, 0, [0, 0, 2], [0, 4], [9, 4], 0)
    assert length == [0xffffffff, 0] and pos == [0, 0xfffffffb]
    # fill: lists and positions of another batch - every byte of [out_off[0], out_off[n]) is still written once, nothing else, and no
    # input byte outside an item is read (FillReplay reads self.text[b + src] only for src < the item's length: else 0)
    rng = random.Random(SEED + 22)
    items = [bytes(rng.choice(b"abc") for _ in range(rng.randrange(12))) for _ in range(100)]
    first, start, end = csr_lists([[(0, 1)] * rng.randrange(3) for _ in items])
    pos = [rng.randrange(40) for _ in start]
    end = [rng.randrange(40) for _ in start]
    text, offs = pack(items, 1, 3)
    out_off = [2]
    for _ in items:
        out_off.append(out_off[-1] + rng.randrange(30))
    out = bytearray([POISON]) * (out_off[-1] + MARGIN)
    f = FillReplay(text.tolist(), offs, 1, first, end, pos, b"RR", out_off, out, 3)
    f.run()
    assert all(f.written[2:out_off[-1]]) and not any(f.written[:2]) and not any(f.written[out_off[-1]:])


def test_arguments_are_checked_without_a_device():
    r = rr.RRegex("ab+c")
    L, C = rr._L, rr.C
    p = C.cast((C.c_uint64 * 8)(), C.c_void_p)
    tot = C.byref(C.c_size_t(0))
    ARG, UNSUPPORTED = 2, 4
    # rrx_replace_matches_sizes(device, off, nitems, trim, first, start, end, rep_len, len, pos, stream)
    ok = [0, p, 5, 0, p, p, p, 2, p, p, None]
    for k in (1, 4, 5, 6, 8, 9):
        a = list(ok)
        a[k] = None
        assert L.rrx_replace_matches_sizes(*a) == ARG, k
        assert b"null" in L.rrx_last_error()
    assert L.rrx_replace_matches_sizes(0, None, 0, 0, None, None, None, 2, None, None, None) == 0          # nitems == 0: nothing to do
    # rrx_replace_matches_fill(device, bytes, off, nitems, trim, first, end, pos, rep, rep_len, out_off, out, stream)
    ok = [0, p, p, 5, 0, p, p, p, p, 2, p, p, None]
    for k in (2, 5, 6, 7, 8, 10):
        a = list(ok)
        a[k] = None
        assert L.rrx_replace_matches_fill(*a) == ARG, k
    assert L.rrx_replace_matches_fill(0, None, None, 0, 0, None, None, None, None, 0, None, None, None) == 0
    # rrx_replace_all_longest_extents(re, device, bytes, off, nitems, trim, rep, rep_len, out_off, out, cap, total, stream)
    ok = [r._h, 0, p, p, 5, 0, b"xy", 2, p, p, 9, tot, None]
    for k in (0, 3, 6, 8, 9, 11):
        a = list(ok)
        a[k] = None
        assert L.rrx_replace_all_longest_extents(*a) == ARG, k
    assert L.rrx_replace_all_longest_extents(r._h, 0, None, None, 0, 0, None, 0, None, None, 0, tot, None) == ARG       # no d_out_off, for an empty batch too
    # rrx_replace_all_longest_items(re, items, rep, rep_len, out_off, out, cap, total, stream)
    assert L.rrx_replace_all_longest_items(None, None, b"xy", 2, p, p, 9, tot, None) == ARG
    assert L.rrx_replace_all_longest_items(r._h, None, b"xy", 2, p, p, 9, tot, None) == ARG                # no items handle
    assert b"null" in L.rrx_last_error()
    # a regex without leftmost-longest tables is reported for an empty batch, without a device
    bad = rr.RRegex(EXPLODING)
    assert bad.program(rr.PROGRAM_SEARCH_STARTS) is None
    assert L.rrx_replace_all_longest_extents(bad._h, 0, None, None, 0, 0, b"xy", 2, p, None, 0, tot, None) == UNSUPPORTED
    assert b"determinise" in L.rrx_last_error()
