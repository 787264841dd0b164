"""rrx_replace_matches_sizes / _fill and rrx_replace_all_longest_extents / _items on the device: the replaced column, byte for byte,
and its offsets - against the splice rule on the oracle's lists (short items: the CPU test's patterns, items and expected lists),
against the splice of the lists the device itself found taken earliest-end-first, and against re.sub where Python's greedy search
names the leftmost-longest list (test_search_all_longest_items_lowering checks that).  Every output buffer stands between 64
poisoned bytes in front and 64 behind, which must come back unchanged."""
import ctypes as C
import random
import re

import numpy as np
import pytest

import roaringregex_amd as rr
from test_replace_items_lowering import REPLACEMENTS, splice
from test_search_all_longest_items_lowering import GREEDY_ALL_RE, finditer_all, pack, reference_all
from test_search_all_longest_items_gpu import POOL, pooled_batch, to_dev

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

POISON = 0x5A
GUARD = 64
MAX_BLOCKS_REPLACE = 512 * 1024                     # device.hpp: kReplaceMaxBlocks workgroups of 1024 lanes, then the grid strides


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"


def ptr(t):
    return C.c_void_p(t.data_ptr() if t.numel() else 0)


def poisoned_words(n):
    return torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")


def at_residue(host, mis):
    """A device copy of a host uint8 array whose first byte sits `mis` bytes behind a 16-byte boundary."""
    buf = torch.empty(len(host) + 16, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[mis:mis + len(host)]
    if len(host):
        view.copy_(torch.from_numpy(np.array(host, dtype=np.uint8)))
    return view


class Guarded:
    """`size` output bytes that begin `lead` bytes into d_out, d_out at an address `mis` mod 4, all of it poisoned, with GUARD
    poisoned bytes in front of d_out + lead and behind the last byte."""

    def __init__(self, size, lead=0, mis=0):
        self.buf = torch.full((GUARD + 16 + lead + size + GUARD,), POISON, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.at = GUARD + (mis - GUARD) % 4 + 4                     # (GUARD bytes at least in front, whatever `lead`)
        self.d_out = self.buf[self.at:]
        assert self.d_out.data_ptr() % 4 == mis
        self.lo, self.hi = self.at + lead, self.at + lead + size

    def written(self, what):
        """The output bytes (numpy), after the check that nothing else changed."""
        host = self.buf.cpu().numpy()
        assert (host[:self.lo] == POISON).all() and (host[self.hi:] == POISON).all(), (what, "a byte outside the output was written")
        return host[self.lo:self.hi]

    def untouched(self, what):
        assert bool((self.buf == POISON).all()), (what, "d_out was written")


def expected_column(items, lists, rep, out_first=0):
    outs = [splice(it, w, rep) for it, w in zip(items, lists)]
    off = np.concatenate([[out_first], out_first + np.cumsum([len(o) for o in outs], dtype=np.int64)]).astype(np.int64)
    return np.frombuffer(b"".join(outs), dtype=np.uint8), off


def assert_column(got_bytes, got_off, want_bytes, want_off, what):
    assert np.array_equal(got_off, want_off), (what, "out_off", int(np.nonzero(got_off != want_off)[0][0]))
    assert len(got_bytes) == len(want_bytes), (what, len(got_bytes), len(want_bytes))
    bad = np.nonzero(got_bytes != want_bytes)[0]
    assert bad.size == 0, (what, "first bad byte", int(bad[0]), "item", int(np.searchsorted(want_off, bad[0] + want_off[0], side="right")) - 1,
                           bytes(got_bytes[bad[0]:bad[0] + 8]), bytes(want_bytes[bad[0]:bad[0] + 8]))


def generic_pair(dev, doff, trim, first, start, end, rep, want, what, out_first=0, out_mis=0, rep_mis=0):
    """sizes, the prefix with torch, fill - through the C entries, every buffer of the caller's poisoned; `want` = (bytes, out_off)."""
    L, s = rr._L, rr._stream_ptr(None)
    n, nslots = doff.numel() - 1, max(int(start.numel()), 1)
    if not start.numel():
        start = end = torch.zeros(1, dtype=torch.int32, device="cuda")
    length, pos = poisoned_words(n + 1), poisoned_words(nslots + 1)
    rr._check(L.rrx_replace_matches_sizes(0, ptr(doff), n, trim, ptr(first), ptr(start), ptr(end), len(rep), ptr(length), ptr(pos), s))
    assert int(length[n]) == 0x5A5A5A5A and int(pos[nslots]) == 0x5A5A5A5A, (what, "sizes wrote behind its arrays")
    out_off = torch.full((n + 1,), out_first, dtype=torch.int64, device="cuda")
    out_off[1:] += torch.cumsum(length[:n].to(torch.int64) & 0xFFFFFFFF, dim=0)
    total = int(out_off[-1]) - out_first
    assert total == len(want[0]), (what, "total", total, len(want[0]))
    g = Guarded(total, lead=out_first, mis=out_mis)
    d_rep = at_residue(np.frombuffer(rep, dtype=np.uint8), rep_mis)
    rr._check(L.rrx_replace_matches_fill(0, ptr(dev), ptr(doff), n, trim, ptr(first), ptr(end), ptr(pos), ptr(d_rep), len(rep), ptr(out_off),
                                         ptr(g.d_out) if total else None, s))
    torch.cuda.synchronize()
    assert_column(g.written(what), out_off.cpu().numpy(), want[0], want[1], what)


def one_call(r, dev, doff, trim, rep, want, what, handle=None, out_mis=0):
    """The one-call form with cap = the exact size, on the offsets or on an indexed batch; `want` = (bytes, out_off from 0)."""
    L, s = rr._L, rr._stream_ptr(None)
    n, total = doff.numel() - 1, len(want[0])
    out_off = torch.full((n + 2,), -7, dtype=torch.int64, device="cuda")
    g, tot = Guarded(total, mis=out_mis), C.c_size_t(99)
    d_out = ptr(g.d_out) if total else None
    if handle is None:
        rr._check(L.rrx_replace_all_longest_extents(r._h, 0, ptr(dev), ptr(doff), n, trim, rep, len(rep), ptr(out_off), d_out, total, C.byref(tot), s))
    else:
        rr._check(L.rrx_replace_all_longest_items(r._h, handle._h, rep, len(rep), ptr(out_off), d_out, total, C.byref(tot), s))
    assert tot.value == total and int(out_off[n + 1]) == -7, (what, tot.value, total)
    assert_column(g.written(what), out_off[:n + 1].cpu().numpy(), want[0], want[1], what)


def host_lists(first, start, end):
    f, s, e = first.cpu().numpy(), start.cpu().numpy(), end.cpu().numpy()
    return [list(zip(s[f[k]:f[k + 1]].tolist(), e[f[k]:f[k + 1]].tolist())) for k in range(len(f) - 1)]


def test_short_items_against_the_brute_force():
    for p, items, want_lists in reference_all():
        r = rr.RRegex(p)
        for trim in (0, 1):
            dev, doff = to_dev(*pack(items, trim, lead=3 + trim, seed=len(items) + trim))
            assert int(doff[0]) != 0
            handle = rr.Items(dev, doff, trim=trim)
            longest = r.search_all_longest_extents_fused(dev, doff, trim=trim)
            assert host_lists(*longest) == [list(w) for w in want_lists], (p[:30], "the device's lists are the oracle's")
            lazy = r.search_all_extents_fused(dev, doff, trim=trim)
            lazy_lists = host_lists(*lazy)
            for rep in REPLACEMENTS:
                want = expected_column(items, want_lists, rep)
                what = (p[:30], "trim", trim, "rep_len", len(rep))
                generic_pair(dev, doff, trim, *longest, rep, want, what + ("longest lists",))
                generic_pair(dev, doff, trim, *lazy, rep, expected_column(items, lazy_lists, rep), what + ("earliest-end-first lists",))
                one_call(r, dev, doff, trim, rep, want, what + ("one call",))
                one_call(r, dev, doff, trim, rep, want, what + ("one call, indexed",), handle=handle)
            # the Python layer: the same columns
            rep = REPLACEMENTS[2]
            want = expected_column(items, want_lists, rep)
            for out, off in (rr.replace_matches(dev, doff, *longest, rep, trim=trim), r.replace_all_longest_extents(dev, doff, rep, trim=trim),
                             r.replace_all_longest_extents(dev, doff, rep, trim=trim, cap=1), r.replace_all_longest_items(handle, rep)):
                assert_column(out.cpu().numpy(), off.cpu().numpy(), want[0], want[1], (p[:30], "python", trim))
    for p, item, want in (("a*", b"baab", b"<>b<><>b<>"), ("[0-9]+", b"a1 22 333", b"a<> <> <>"), ("ab|b+", b"abbbab", b"<><><>")):
        dev, doff = to_dev(*pack([item] * 3, 1, lead=3))
        out, off = rr.RRegex(p).replace_all_longest_extents(dev, doff, b"<>", trim=1)
        assert out.cpu().numpy().tobytes() == want * 3 and off.tolist() == [0, len(want), 2 * len(want), 3 * len(want)], (p, "named case")


def pooled_column(per, idx, out_first=0):
    """The column of a batch drawn from a pool by `idx`, from the output per pool item (numpy: the batch may pass half a million)."""
    flat = np.frombuffer(b"".join(per), dtype=np.uint8)
    plen = np.array([len(x) for x in per], dtype=np.int64)
    poff = np.concatenate([[0], np.cumsum(plen)[:-1]])
    lens = plen[idx]
    off = np.concatenate([[0], np.cumsum(lens)])
    src = np.arange(int(off[-1]), dtype=np.int64) - np.repeat(off[:-1], lens) + np.repeat(poff[idx], lens)
    return flat[src], (off + out_first).astype(np.int64)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, MAX_BLOCKS_REPLACE + 65])
def test_batch_sizes(n):
    """Wave edges, workgroup edges and more items than one pass of the fill grid holds; trim 3 is larger than some items (region =
    item + ';'); an empty replacement shrinks whole-matched items to nothing, a long one makes items grow."""
    p, trim, lead = "ab+c", 3, 16
    r = rr.RRegex(p)
    trimmed = [(it + b";")[:max(len(it) + 1 - trim, 0)] for it in POOL]
    assert len(POOL) == 14 and sum(not t for t in trimmed) >= 3
    text, off, idx = pooled_batch(n, 40 + n % 7, lead)
    dev, doff = to_dev(text, off)
    lists = r.search_all_longest_extents_fused(dev, doff, trim=trim)
    handle = rr.Items(dev, doff, trim=trim) if n <= 1025 else None
    for rep in (b"", b"<--ab+c-->"):
        per = [re.sub(GREEDY_ALL_RE[p], lambda m: rep, it) for it in trimmed]
        assert per == [splice(it, finditer_all(p, it), rep) for it in trimmed]
        if rep:
            assert any(len(o) > len(t) for o, t in zip(per, trimmed)) and any(len(o) < len(t) for o, t in zip(per, trimmed))
        else:
            assert any(t and not o for o, t in zip(per, trimmed)) and any(o for o in per)
        want = pooled_column(per, idx, out_first=9)
        generic_pair(dev, doff, trim, *lists, rep, want, ("batch", n, len(rep)), out_first=9, out_mis=n % 4)
        want = pooled_column(per, idx)
        one_call(r, dev, doff, trim, rep, want, ("batch", n, len(rep), "one call"), out_mis=(n + 1) % 4)
        if handle is not None:
            one_call(r, dev, doff, trim, rep, want, ("batch", n, len(rep), "one call, indexed"), handle=handle)


def test_alignment():
    """Pass boundaries d_out_off[F] on all four residues mod 4 (the address counted in), d_out, d_bytes and d_rep at addresses 1, 2
    and 3 mod 4, d_out_off[0] = 5 in the generic form, rep_len 1, 3, 4 and 5."""
    p = "ab+c"
    r = rr.RRegex(p)
    rng = random.Random(51)
    items = []
    for k in range(64 * 9 + 11):                                    # ten passes of a wave, the last one partial
        filler = bytes(rng.choice(b"xyz ") for _ in range(rng.randrange(0, 9)))
        items.append(filler + (b"abbc" if k % 3 == 0 else b"") + filler[:k % 4] + (b"abc" if k % 5 == 0 else b""))
    # every whole pass: a multiple of four matches and 1 mod 4 bytes outside them - its output has 1 mod 4 bytes whatever rep_len is,
    # so the passes begin at every residue in turn
    for first in range(0, 64 * 9, 64):
        matches = sum(len(finditer_all(p, it)) for it in items[first:first + 64])
        items[first + 1] += b"abc" * (-matches % 4)
        outside = len(re.sub(GREEDY_ALL_RE[p], b"", b"".join(items[first:first + 64])))
        items[first + 1] += b"x" * ((1 - outside) % 4)
    lists = [finditer_all(p, it) for it in items]
    text, offs = pack(items, 1, lead=0)
    for m in (1, 2, 3):
        dev = at_residue(text, m)
        doff = torch.from_numpy(offs).cuda()
        assert dev.data_ptr() % 4 == m
        found = r.search_all_longest_extents_fused(dev, doff, trim=1)
        assert host_lists(*found) == lists
        for rep in (b"R", b"RST", b"RSTU", b"RSTUV"):
            want = expected_column(items, lists, rep, out_first=5)
            out_mis, rep_mis = m % 3 + 1, (m + 1) % 3 + 1
            residues = {(out_mis + int(o)) % 4 for o in want[1][::64]}
            assert residues == {0, 1, 2, 3}, (m, rep, residues)
            generic_pair(dev, doff, 1, *found, rep, want, ("alignment", m, rep), out_first=5, out_mis=out_mis, rep_mis=rep_mis)
            want = expected_column(items, lists, rep)
            one_call(r, dev, doff, 1, rep, want, ("alignment, one call", m, rep), out_mis=m)
            one_call(r, dev, doff, 1, rep, want, ("alignment, one call, indexed", m, rep), handle=rr.Items(dev, doff, trim=1), out_mis=out_mis)


def test_long_items():
    """One item of 60000 digits and blanks with more than 10000 matches, one match of 30 KB, a 100 KB item without a match, a batch
    of a single item; the expected columns from re.sub."""
    rng = random.Random(41)
    fill = b"xy zb" * 20001                                         # (no 'a', no digit: no pattern matches inside it)
    dense = bytes(rng.choice(b"0123456789   ") for _ in range(60000))
    assert len(finditer_all("[0-9]+", dense)) > 10000
    long_match = fill[:40000] + b"a" + b"b" * 30000 + b"c" + fill[:16] + b"abc"
    assert max(e - s for s, e in finditer_all("ab+c", long_match)) == 30002
    batches = (("[0-9]+", [dense, fill[:100000], b"12345" + fill[:65536] + b"678"]), ("[0-9]+", [dense]), ("[0-9]+", [fill[:100000]]),
               ("ab+c", [long_match, fill[:100000], b"abc" * 2000]), ("ab+c", [long_match]))
    for p, items in batches:
        r = rr.RRegex(p)
        lists = [finditer_all(p, it) for it in items]
        for (trim, lead), rep in zip(((0, 0), (1, 7)), (b"#", REPLACEMENTS[3])):
            dev, doff = to_dev(*pack(items, trim, lead, seed=trim))
            outs = [re.sub(GREEDY_ALL_RE[p], lambda m: rep, it) for it in items]
            assert outs == [splice(it, w, rep) for it, w in zip(items, lists)]
            want = (np.frombuffer(b"".join(outs), dtype=np.uint8), np.concatenate([[0], np.cumsum([len(o) for o in outs])]).astype(np.int64))
            found = r.search_all_longest_extents_fused(dev, doff, trim=trim)
            what = (p, "long", len(items), trim)
            generic_pair(dev, doff, trim, *found, rep, want, what, out_mis=1)
            one_call(r, dev, doff, trim, rep, want, what + ("one call",), out_mis=3)
            one_call(r, dev, doff, trim, rep, want, what + ("one call, indexed",), handle=rr.Items(dev, doff, trim=trim))


def test_degenerate_cases():
    L, s = rr._L, rr._stream_ptr(None)
    r = rr.RRegex("ab+c")
    nothing = torch.empty(0, dtype=torch.uint8, device="cuda")
    zero = torch.zeros(1, dtype=torch.int64, device="cuda")
    # nitems == 0: the generic entries write nothing, the one-call forms d_out_off[0] = 0
    g, w = Guarded(8), poisoned_words(4)
    assert L.rrx_replace_matches_sizes(0, ptr(zero), 0, 0, ptr(zero), ptr(w), ptr(w), 2, ptr(w), ptr(w), s) == 0
    assert L.rrx_replace_matches_fill(0, None, ptr(zero), 0, 0, ptr(zero), ptr(w), ptr(w), ptr(g.d_out), 2, ptr(zero), ptr(g.d_out), s) == 0
    torch.cuda.synchronize()
    g.untouched("empty batch")
    assert bool((w == 0x5A5A5A5A).all())
    for rx in (r, rr.RRegex("a*"), rr.RRegex("[]")):
        one_call(rx, nothing, zero, 0, b"xy", (np.empty(0, dtype=np.uint8), np.zeros(1, dtype=np.int64)), "empty batch")
        one_call(rx, nothing, zero, 0, b"xy", (np.empty(0, dtype=np.uint8), np.zeros(1, dtype=np.int64)), "empty batch, indexed", handle=rr.Items(nothing, zero))
        out, off = rx.replace_all_longest_extents(nothing, zero, b"xy")
        assert out.numel() == 0 and off.tolist() == [0]
    # a batch of empty items: nothing but offsets; a nullable pattern inserts R into each
    off0 = torch.zeros(71, dtype=torch.int64, device="cuda")
    empties = [b""] * 70
    for rx, lists in ((r, [[]] * 70), (rr.RRegex("a*"), [[(0, 0)]] * 70), (rr.RRegex("[]"), [[]] * 70)):
        for rep in (b"", b"xyz"):
            want = expected_column(empties, lists, rep)
            one_call(rx, nothing, off0, 0, rep, want, ("empty items", rx.pattern, rep))
            generic_pair(nothing, off0, 0, *rx.search_all_longest_extents_fused(nothing, off0), rep, want, ("empty items, generic", rx.pattern, rep))
    # R = b"" on items that are matched whole: *total == 0, d_out null
    items = [b"abc", b"abbbc", b"abcabbc", b""] * 40
    dev, doff = to_dev(*pack(items, 1, lead=2))
    want = expected_column(items, [finditer_all("ab+c", it) for it in items], b"")
    assert len(want[0]) == 0
    one_call(r, dev, doff, 1, b"", want, "matched whole")
    one_call(r, dev, doff, 1, b"", want, "matched whole, indexed", handle=rr.Items(dev, doff, trim=1))
    generic_pair(dev, doff, 1, *r.search_all_longest_extents_fused(dev, doff, trim=1), b"", want, "matched whole, generic")
    # a pattern that accepts the empty string: re.sub; the empty language: the items without their separators
    rng = random.Random(52)
    items = [bytes(rng.choice(b"aab") for _ in range(rng.randrange(0, 40))) for _ in range(150)] + [b"baab", b""]
    for trim, lead in ((0, 0), (1, 5), (2, 1)):
        dev, doff = to_dev(*pack(items, trim, lead))
        handle = rr.Items(dev, doff, trim=trim)
        for rep in (b"", b"<>", REPLACEMENTS[3]):
            outs = [re.sub(rb"a*", lambda m: rep, it) for it in items]
            want = (np.frombuffer(b"".join(outs), dtype=np.uint8), np.concatenate([[0], np.cumsum([len(o) for o in outs])]).astype(np.int64))
            one_call(rr.RRegex("a*"), dev, doff, trim, rep, want, ("a*", trim, rep[:4]))
            one_call(rr.RRegex("a*"), dev, doff, trim, rep, want, ("a*, indexed", trim, rep[:4]), handle=handle)
            want = expected_column(items, [[]] * len(items), rep)
            assert want[0].tobytes() == b"".join(items)
            one_call(rr.RRegex("[]"), dev, doff, trim, rep, want, ("[]", trim, rep[:4]))
            one_call(rr.RRegex("[]"), dev, doff, trim, rep, want, ("[], indexed", trim, rep[:4]), handle=handle)
    # a trim larger than every item: an empty column
    one_call(r, dev, doff, 100, b"xy", expected_column([b""] * len(items), [[]] * len(items), b"xy"), "a trim larger than every item")


def test_the_cap_protocol():
    L, s = rr._L, rr._stream_ptr(None)
    p, items, want_lists = next(x for x in reference_all() if x[0] == "[ab]{1,2}b*a*")
    r = rr.RRegex(p)
    dev, doff = to_dev(*pack(items, 1, lead=1))
    handle = rr.Items(dev, doff, trim=1)
    n, rep = len(items), b"<<>>"
    want = expected_column(items, want_lists, rep)
    total = len(want[0])
    assert total > 2 * n
    for indexed in (False, True):
        for cap in (total - 1, 0, total, total + 5):
            g, tot = Guarded(total), C.c_size_t(99)
            out_off = torch.full((n + 2,), -7, dtype=torch.int64, device="cuda")
            d_out = ptr(g.d_out) if cap else None
            if indexed:
                rr._check(L.rrx_replace_all_longest_items(r._h, handle._h, rep, len(rep), ptr(out_off), d_out, cap, C.byref(tot), s))
            else:
                rr._check(L.rrx_replace_all_longest_extents(r._h, 0, ptr(dev), ptr(doff), n, 1, rep, len(rep), ptr(out_off), d_out, cap, C.byref(tot), s))
            torch.cuda.synchronize()
            assert tot.value == total and int(out_off[n + 1]) == -7 and np.array_equal(out_off[:n + 1].cpu().numpy(), want[1]), (indexed, cap, "d_out_off is complete either way")
            if cap < total:
                g.untouched((indexed, cap))
            else:
                assert np.array_equal(g.written((indexed, cap)), want[0]), (indexed, cap)
    assert L.rrx_replace_all_longest_extents(r._h, 0, ptr(dev), ptr(doff), n, 1, rep, len(rep), ptr(out_off), None, 5, C.byref(tot), s) == 2      # RRX_ERR_ARG: cap > 0 and no d_out


TOO_LONG = b"an output item of 2^30 bytes or more: use rrx_search_all_longest_extents and the two passes rrx_replace_matches_sizes / _fill"


@pytest.mark.parametrize("indexed", [False, True])
def test_an_output_item_of_2_30_bytes_is_refused(indexed):
    """The flag word of the one-call form: one item of 65536 b"a", every byte a match of `a`.  A replacement of 16383 bytes gives an
    output item of 65536 * 16383 = 2^30 - 65536 bytes, the largest the scan carries; one of 16384 bytes gives exactly 2^30 and is
    refused, the total left 0.  cap = 0 and no d_out: nothing of that size is allocated.  The flag is the call's own and zeroed per
    call: the next call on the same regex goes through."""
    L, s = rr._L, rr._stream_ptr(None)
    r = rr.RRegex("a")
    dev, doff = to_dev(*pack([b"a" * 65536], 0))
    handle = rr.Items(dev, doff, trim=0)

    def call(rep):
        tot, out_off = C.c_size_t(99), torch.full((2,), -7, dtype=torch.int64, device="cuda")
        if indexed:
            rc = L.rrx_replace_all_longest_items(r._h, handle._h, rep, len(rep), ptr(out_off), None, 0, C.byref(tot), s)
        else:
            rc = L.rrx_replace_all_longest_extents(r._h, 0, ptr(dev), ptr(doff), 1, 0, rep, len(rep), ptr(out_off), None, 0, C.byref(tot), s)
        torch.cuda.synchronize()
        return rc, tot.value, out_off.cpu().tolist()

    assert call(b"r" * 16383) == (0, 65536 * 16383, [0, 65536 * 16383])
    rc, total, _ = call(b"r" * 16384)
    assert (rc, total) == (4, 0) and L.rrx_last_error() == TOO_LONG                        # RRX_ERR_UNSUPPORTED
    assert call(b"r") == (0, 65536, [0, 65536])
