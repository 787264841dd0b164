"""rrx_group_spans_list_*, rrx_replace_template_sizes / _fill and rrx_replace_groups_longest_* on the device: the replaced column,
byte for byte, and its offsets - against the pure-Python splice of test_replace_template_lowering over the brute-force spans (short
items: that test's patterns, items, lists and spans) and, beyond the brute force's reach, over Python's spans on patterns for which
that test shows they are ours.  Every buffer of the caller's - the output, the planes, the marks, d_len, d_pos - is poisoned and
stands between guards that must come back unchanged (test_replace_items_gpu's Guarded for the bytes)."""
import ctypes as C
import random
import re

import numpy as np
import pytest

import roaringregex_amd as rr
from test_replace_items_gpu import Guarded, assert_column, at_residue, host_lists, poisoned_words, ptr
from test_replace_template_lowering import (CASES, DATE, NONE, TEMPLATES, expected_items, parse_py, reference_templates, replay,
                                            span_group, splice_template)
from test_search_all_longest_items_gpu import to_dev
from test_search_all_longest_items_lowering import pack

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

WORD_POISON = 0x5A5A5A5A
GUARD_WORDS = 16


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"


def column(outs, out_first=0):
    off = np.concatenate([[out_first], out_first + np.cumsum([len(o) for o in outs], dtype=np.int64)]).astype(np.int64)
    return np.frombuffer(b"".join(outs), dtype=np.uint8), off


def fits(repl, ngroups):
    return all(not isinstance(s, int) or s <= ngroups for s in parse_py(repl))


@pytest.fixture(scope="module")
def handles():
    """{pattern: [RGroup of group 1, 2 ...]} of the reference's patterns, compiled once."""
    return {p: [rr.RGroup(p, g) for g in range(1, ngroups + 1)] for p, ngroups, _, _ in CASES}


def shifted_lists(first, start, end, first0):
    """The device's match list moved to begin at slot first0: the slots in front are somebody else's (poisoned)."""
    total = int(first[-1])
    s, e = poisoned_words(first0 + total + 1), poisoned_words(first0 + total + 1)
    s[first0:first0 + total] = start[:total]
    e[first0:first0 + total] = end[:total]
    return first + first0, s, e, total


def planes_of(groups, refs, dev, doff, trim, first, start, end, first0, total, stride, what, handle=None, in_place=False):
    """rrx_group_spans_list_* into one plane per referenced group: plane r, slot q at r * stride + q.  Planes and marks are poisoned;
    exactly the slots first0 .. first0 + total of every plane and no mark word at or beyond marks_words may change."""
    L, s = rr._L, rr._stream_ptr(None)
    n = doff.numel() - 1
    words = L.rrx_search_all_longest_marks_words(dev.numel(), n)
    marks = poisoned_words(words + GUARD_WORDS)
    size = max(len(refs), 1) * stride + GUARD_WORDS
    ref_start, ref_end = poisoned_words(size), poisoned_words(size)
    for r, g in enumerate(refs):
        ps, pe = ref_start[r * stride:], ref_end[r * stride:]
        src_s, src_e = start, end
        if in_place:                                                # the plane holds the list: the entry overwrites it
            ps[:first0 + total] = start[:first0 + total]
            pe[:first0 + total] = end[:first0 + total]
            src_s, src_e = ps, pe
        if handle is None:
            rr._check(L.rrx_group_spans_list_extents(groups[g - 1]._h, 0, ptr(dev), ptr(doff), n, trim, ptr(first), ptr(src_s), ptr(src_e), ptr(marks), words,
                                                     ptr(ps), ptr(pe), s))
        else:
            rr._check(L.rrx_group_spans_list_items(groups[g - 1]._h, handle._h, ptr(first), ptr(src_s), ptr(src_e), ptr(marks), words, ptr(ps), ptr(pe), s))
    torch.cuda.synchronize()
    assert bool((marks[words:] == WORD_POISON).all()), (what, "a mark word at or beyond marks_words was written")
    for plane in (ref_start, ref_end):
        host = plane.cpu().numpy()
        for r in range(len(refs)):
            row = host[r * stride:(r + 1) * stride]
            assert (row[:first0] == WORD_POISON).all() and (row[first0 + total:] == WORD_POISON).all(), (what, "a slot outside the list was written", r)
        assert (host[max(len(refs), 1) * stride:] == WORD_POISON).all() and (len(refs) or (host == WORD_POISON).all()), (what, "behind the planes")
    return ref_start, ref_end


def plane_lists(plane_start, plane_end, refs, first, stride):
    """The planes as {g: [[(i, j) per match] per item]}."""
    f = first.cpu().numpy()
    out = {}
    for r, g in enumerate(refs):
        s, e = plane_start[r * stride:].cpu().numpy(), plane_end[r * stride:].cpu().numpy()
        out[g] = [list(zip(s[f[k]:f[k + 1]].tolist(), e[f[k]:f[k + 1]].tolist())) for k in range(len(f) - 1)]
    return out


def generic(groups, repl, dev, doff, trim, want, what, first0=0, extra_stride=0, out_first=0, out_mis=0, handle=None, in_place=False, lists=None,
            want_spans=None):
    """search, list spans into planes, sizes, the prefix with torch, fill - through the C entries; `want` = (bytes, out_off)."""
    L, s = rr._L, rr._stream_ptr(None)
    n = doff.numel() - 1
    tpl = rr.Template(repl)
    refs = tpl.refs
    lead = next(g for g in groups if g is not None)
    found = lists if lists is not None else lead.regex.search_all_longest_extents_fused(dev, doff, trim=trim)
    first, start, end, total = shifted_lists(*found, first0)
    stride = first0 + total + extra_stride
    ref_start, ref_end = planes_of(groups, refs, dev, doff, trim, first, start, end, first0, total, max(stride, 1), what, handle, in_place)
    if want_spans is not None:
        got = plane_lists(ref_start, ref_end, refs, first, max(stride, 1))
        for g in refs:
            assert got[g] == [list(w) for w in want_spans[g]], (what, "the spans of group", g)
    length, pos = poisoned_words(n + 1), poisoned_words(first0 + total + 1)
    rr._check(L.rrx_replace_template_sizes(0, ptr(doff), n, trim, ptr(first), ptr(start), ptr(end), tpl._h, ptr(ref_start), ptr(ref_end), max(stride, 1),
                                           ptr(length), ptr(pos), s))
    assert int(length[n]) == WORD_POISON and int(pos[first0 + total]) == WORD_POISON and bool((pos[:first0] == WORD_POISON).all()), (what, "sizes wrote outside its slots")
    out_off = torch.full((n + 1,), out_first, dtype=torch.int64, device="cuda")
    out_off[1:] += torch.cumsum(length[:n].to(torch.int64) & 0xFFFFFFFF, dim=0)
    size = int(out_off[-1]) - out_first
    assert size == len(want[0]), (what, "total", size, len(want[0]))
    g = Guarded(size, lead=out_first, mis=out_mis)
    rr._check(L.rrx_replace_template_fill(0, ptr(dev), ptr(doff), n, trim, ptr(first), ptr(start), ptr(end), ptr(pos), tpl._h, ptr(ref_start), ptr(ref_end),
                                          max(stride, 1), ptr(out_off), ptr(g.d_out) if size else None, s))
    torch.cuda.synchronize()
    assert_column(g.written(what), out_off.cpu().numpy(), want[0], want[1], what)


def one_call(groups, repl, dev, doff, trim, want, what, handle=None, out_mis=0):
    """The one-call form with cap = the exact size; `want` = (bytes, out_off from 0)."""
    L, s = rr._L, rr._stream_ptr(None)
    n, total = doff.numel() - 1, len(want[0])
    tpl = rr.Template(repl)
    h = rr._group_handles(groups)
    out_off = torch.full((n + 2,), -7, dtype=torch.int64, device="cuda")
    g, tot = Guarded(total, mis=out_mis), C.c_size_t(99)
    d_out = ptr(g.d_out) if total else None
    if handle is None:
        rr._check(L.rrx_replace_groups_longest_extents(h, len(groups), tpl._h, 0, ptr(dev), ptr(doff), n, trim, ptr(out_off), d_out, total, C.byref(tot), s))
    else:
        rr._check(L.rrx_replace_groups_longest_items(h, len(groups), tpl._h, handle._h, ptr(out_off), d_out, total, C.byref(tot), s))
    assert tot.value == total and int(out_off[n + 1]) == -7, (what, tot.value, total)
    assert_column(g.written(what), out_off[:n + 1].cpu().numpy(), want[0], want[1], what)


def test_short_items_against_the_brute_force(handles):
    for n_p, (p, ngroups, items, lists, spans) in enumerate(reference_templates()):
        groups = handles[p]
        for trim in (0, 1):
            dev, doff = to_dev(*pack(items, trim, lead=3 + trim, seed=len(items) + trim))
            assert int(doff[0]) != 0
            handle = rr.Items(dev, doff, trim=trim)
            found = groups[0].regex.search_all_longest_extents_fused(dev, doff, trim=trim)
            assert host_lists(*found) == [list(w) for w in lists], (p, "the device's lists are the oracle's")
            for n_t, repl in enumerate(t for t in TEMPLATES if fits(t, ngroups)):
                outs = expected_items(items, lists, spans, repl)
                what = (p, "trim", trim, repl[:12])
                generic(groups, repl, dev, doff, trim, column(outs, out_first=n_t), what + ("generic",), first0=(n_p + n_t) % 3, extra_stride=n_t % 2 * 7,
                        out_first=n_t, out_mis=(n_p + n_t) % 4, handle=handle if n_t % 2 else None, in_place=bool(n_t % 3 == 1), lists=found, want_spans=spans)
                one_call(groups, repl, dev, doff, trim, column(outs), what + ("one call",), out_mis=n_t % 4)
                one_call(groups, repl, dev, doff, trim, column(outs), what + ("one call, indexed",), handle=handle)
                if repl == rb"\0":                                  # the input column without its separators: no oracle needed
                    assert b"".join(outs) == b"".join(items)
                if b"\\" not in repl:                               # a literal: the literal entries' column, byte for byte
                    out, off = rr.replace_matches(dev, doff, *found, repl, trim=trim)
                    assert_column(out.cpu().numpy(), off.cpu().numpy(), *column(outs), what + ("rrx_replace_matches_*",))
            # the Python layer: the same columns; a handle may be left out where the template does not reference its group
            repl = TEMPLATES[3] if ngroups < 2 else TEMPLATES[4]
            want = column(expected_items(items, lists, spans, repl))
            assert found[1].numel() > 0
            planes = [groups[g - 1].spans_list_extents(dev, doff, *found, trim=trim) for g in rr.Template(repl).refs]
            cat = lambda k: torch.cat([pl[k] for pl in planes])
            for out, off in (rr.replace_template(dev, doff, *found, rr.Template(repl), cat(0), cat(1), trim=trim),
                             rr.replace_groups_longest_extents(groups, repl, dev, doff, trim=trim),
                             rr.replace_groups_longest_extents(groups, rr.Template(repl), dev, doff, trim=trim, cap=1),
                             rr.replace_groups_longest_items(groups, repl, handle)):
                assert_column(out.cpu().numpy(), off.cpu().numpy(), want[0], want[1], (p, "python", trim))
            if ngroups >= 2:
                out, off = rr.replace_groups_longest_extents([groups[0]] + [None] * (ngroups - 1), rb"<\1>", dev, doff, trim=trim)
                assert_column(out.cpu().numpy(), off.cpu().numpy(), *column(expected_items(items, lists, spans, rb"<\1>")), (p, "one handle", trim))
    dev, doff = to_dev(*pack([b"on 12/31/1999."] * 3, 1, lead=3))
    out, off = rr.replace_groups_longest_extents(handles[DATE], rb"\3-\1-\2", dev, doff, trim=1)
    assert out.cpu().numpy().tobytes() == b"on 1999-12-31." * 3 and off.tolist() == [0, 14, 28, 42], "the named case"


# a pool for the batches: items with 0, 1, 2 and 33 matches, adjacent matches, empty items; beyond the brute force's 22 bytes the
# spans are Python's (test_replace_template_lowering.test_against_re_sub: they are ours for this pattern)
POOL = [b"", b"x", b"1/2/3", b"on 12/31/1999.", b"1/2/3 10/20/1999x", b"", b"9/9/99/9/9", b"no date / here 1/2", b" ".join(b"%d/%d/%d" % (k, k + 1, 1990 + k) for k in range(33)),
        b"1/2/34/5/6", b"77/8/9", b"/1/2/3/"]


def pool_batch(pool, n, seed, lead, trim):
    """n items drawn from `pool` (all of it, where n allows), each followed by `trim` separator bytes -> (text, offsets, index into
    the pool per item)."""
    rng = np.random.default_rng(seed)
    regions = [it + b";" * trim for it in pool]
    flat = np.frombuffer(b"".join(regions), dtype=np.uint8)
    rlen = np.array([len(x) for x in regions], dtype=np.int64)
    roff = np.concatenate([[0], np.cumsum(rlen)[:-1]])
    idx = rng.integers(0, len(pool), size=n)
    if n >= len(pool):
        idx[:len(pool)] = np.arange(len(pool))
    lens = rlen[idx]
    off = np.concatenate([[0], np.cumsum(lens)])
    src = np.arange(int(off[-1]), dtype=np.int64) - np.repeat(off[:-1], lens) + np.repeat(roff[idx], lens)
    text = np.concatenate([np.full(lead, ord("q"), dtype=np.uint8), flat[src]])
    return text, (off + lead).astype(np.int64), idx


def pooled_column(per, idx, out_first=0):
    flat = np.frombuffer(b"".join(per), dtype=np.uint8)
    plen = np.array([len(x) for x in per], dtype=np.int64)
    poff = np.concatenate([[0], np.cumsum(plen)[:-1]])
    lens = plen[idx]
    off = np.concatenate([[0], np.cumsum(lens)])
    src = np.arange(int(off[-1]), dtype=np.int64) - np.repeat(off[:-1], lens) + np.repeat(poff[idx], lens)
    return flat[src], (off + out_first).astype(np.int64)


def python_reference(p, ngroups, items):
    rx = re.compile(p.encode())
    lists = [[m.span() for m in rx.finditer(it)] for it in items]
    spans = {g: [[m.span(g) for m in rx.finditer(it)] for it in items] for g in range(1, ngroups + 1)}
    return lists, spans


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_batch_sizes(n, handles):
    """Wave edges and more items than a workgroup holds, both trims, empty items in between, items with 0, 1, 2 and 33 matches;
    every template on each; d_first[0], d_out_off[0] not 0 and planes wider than the list."""
    groups = handles[DATE]
    for trim in (0, 1):
        pool = POOL if trim else [it + b" " if it else it for it in POOL]      # (every item ends in a blank of its own there; empty ones stay empty)
        lists, spans = python_reference(DATE, 3, pool)
        assert {len(w) for w in lists} >= {0, 1, 2, 33}
        short = [k for k, it in enumerate(pool) if len(it) <= 22]
        assert all([span_group(DATE, g, pool[k], s, e) for s, e in lists[k]] == spans[g][k] for k in short for g in (1, 2, 3)), "Python's spans are the brute force's"
        text, off, idx = pool_batch(pool, n, 40 + n % 7, lead=16 + trim, trim=trim)
        dev, doff = to_dev(text, off)
        found = groups[0].regex.search_all_longest_extents_fused(dev, doff, trim=trim)
        handle = rr.Items(dev, doff, trim=trim)
        for n_t, repl in enumerate(TEMPLATES):
            per = expected_items(pool, lists, spans, repl)
            what = ("batch", n, "trim", trim, repl[:12])
            generic(groups, repl, dev, doff, trim, pooled_column(per, idx, out_first=9), what, first0=5, extra_stride=3, out_first=9, out_mis=(n + n_t) % 4, lists=found)
            one_call(groups, repl, dev, doff, trim, pooled_column(per, idx), what + ("one call",), out_mis=(n + 1) % 4)
            if n_t % 3 == 0:
                one_call(groups, repl, dev, doff, trim, pooled_column(per, idx), what + ("one call, indexed",), handle=handle)


def test_empty_groups(handles):
    """A group that is often empty and matches that touch (e_k == s_{k+1}), in batches around a wave's 64 items at trim 0: x(a*)."""
    for p, ngroups, pool in (("x(a*)", 1, [b"", b"x ", b"xaa ", b"xxax ", b"b ", b"axaaaxa x ", b"xa" * 33 + b" "]),):
        groups = handles[p]
        lists, spans = python_reference(p, ngroups, pool)
        assert any(s == e for w in spans[1] for s, e in w) and max(len(w) for w in lists) == 33
        assert any(a[1] == b[0] for w in lists for a, b in zip(w, w[1:])), "adjacent matches: e_k == s_{k+1}"
        assert all([span_group(p, 1, it, s, e) for s, e in w] == sp for it, w, sp in zip(pool, lists, spans[1]) if len(it) <= 22)
        rng = random.Random(7)
        for n in (63, 64, 65):
            items = [rng.choice(pool) for _ in range(n)]
            items[n // 2] = b""
            ref = python_reference(p, ngroups, items)
            dev, doff = to_dev(*pack(items, 0, lead=n % 5))
            for repl in (t for t in TEMPLATES if fits(t, ngroups)):
                outs = expected_items(items, ref[0], ref[1], repl)
                generic(groups, repl, dev, doff, 0, column(outs, out_first=2), (p, n, "trim 0", repl[:12]), first0=1, out_first=2, out_mis=n % 4, want_spans=ref[1])
                one_call(groups, repl, dev, doff, 0, column(outs), (p, n, "trim 0, one call", repl[:12]))


def test_a_replacement_longer_than_a_wave_turn():
    """A group of 1 KB referenced twice: one replacement is eight turns of a wave's 256 bytes, with a literal between the two copies
    at every position inside a dword."""
    p = "x(a+)y"
    groups = [rr.RGroup(p, 1)]
    assert span_group(p, 1, b"bxaaayb", 1, 6) == re.search(p.encode(), b"bxaaayb").span(1) == (2, 5)
    items = [b"b" * k + b"x" + b"a" * 1024 + b"y" + b"xay" * k for k in range(5)] + [b"", b"xa", b"x" + b"a" * 700 + b"yx" + b"a" * 300 + b"y"]
    lists, spans = python_reference(p, 1, items)
    for trim, lead in ((0, 1), (1, 6)):
        dev, doff = to_dev(*pack(items, trim, lead))
        for repl in (rb"\1\1", rb"\1-\1", rb"<<\1>>=\1", rb"\0\1"):
            outs = expected_items(items, lists, spans, repl)
            assert max(len(o) for o in outs) > 2048
            for out_mis in range(4):
                generic(groups, repl, dev, doff, trim, column(outs, out_first=3), ("1 KB group", trim, repl, out_mis), out_first=3, out_mis=out_mis, want_spans=spans)
            one_call(groups, repl, dev, doff, trim, column(outs), ("1 KB group, one call", trim, repl), out_mis=trim + 1)


def test_alignment(handles):
    """d_bytes at all 16 address residues, d_out at all 4; the segments of the replacements begin at all four positions inside a
    dword (the CPU replay of the same batch counts them)."""
    groups = handles[DATE]
    rng = random.Random(61)
    items = [b"x" * (k % 5) + rng.choice(POOL[2:5] + POOL[9:11]) + b" " * (k % 3) for k in range(64 * 2 + 9)]
    lists, spans = python_reference(DATE, 3, items)
    text, offs = pack(items, 1, lead=0)
    repl = rb"[\3-\1-\2]\0"
    outs = expected_items(items, lists, spans, repl)
    got, f = replay(items, lists, spans, repl, trim=1, lead=0, out_first=5, out_addr=1)
    assert got == outs and f.boundaries == {0, 1, 2, 3}
    for mis in range(16):
        dev = at_residue(text, mis)
        doff = torch.from_numpy(offs).cuda()
        assert dev.data_ptr() % 16 == mis
        generic(groups, repl, dev, doff, 1, column(outs, out_first=5), ("alignment", mis), first0=mis % 3, out_first=5, out_mis=mis % 4, want_spans=spans)
        if mis % 5 == 0:
            one_call(groups, repl, dev, doff, 1, column(outs), ("alignment, one call", mis), out_mis=(mis + 1) % 4)


def test_planes_with_no_span_and_in_place_list_spans(handles):
    """A plane entry whose start is 0xFFFFFFFF contributes nothing and one that reaches beyond the item is clamped into it; the list
    entry writes its answers over its own inputs."""
    L, s = rr._L, rr._stream_ptr(None)
    p = "([0-9]+)-([0-9]+)"
    groups = handles[p]
    items = [b"x 12-345 y", b"12-3", b"", b"12-3 4-5", b"7-8"] * 13
    lists, spans = python_reference(p, 2, items)
    dev, doff = to_dev(*pack(items, 1, lead=2))
    n = len(items)
    first, start, end = groups[0].regex.search_all_longest_extents_fused(dev, doff, trim=1)
    assert host_lists(first, start, end) == lists
    separate = [g.spans_list_extents(dev, doff, first, start, end, trim=1) for g in groups]
    in_place = []
    for g in groups:
        a, b = start.clone(), end.clone()
        assert g.spans_list_extents(dev, doff, first, a, b, trim=1, out=(a, b))[0] is a
        in_place.append((a, b))
    torch.cuda.synchronize()
    for g, (sep, inp) in enumerate(zip(separate, in_place), 1):
        assert torch.equal(sep[0], inp[0]) and torch.equal(sep[1], inp[1])
        assert host_lists(first, *sep) == spans[g]
    # a list that is no match list of the pattern: none; a start of ~0u is passed on
    bad_start, bad_end = start.clone(), end.clone()
    k1 = int(first[1])                                              # item 1 is "12-3": [0, 3) is no match of the pattern
    assert (int(start[k1]), int(end[k1])) == (0, 4)
    bad_start[0], bad_end[k1] = -1, 3
    for g in groups:
        got = g.spans_list_extents(dev, doff, first, bad_start, bad_end, trim=1)
        assert (int(got[0][0]), int(got[1][0])) == (-1, -1) and (int(got[0][k1]), int(got[1][k1])) == (-1, -1)
        assert int(got[0][k1 + 1]) >= 0
    # wild planes through the two passes
    tpl = rr.Template(rb"<\1|\2>")
    total = int(first[-1])
    rng = random.Random(9)
    wild = {g: [[(rng.choice([-1, 0, 2, 40, 0x7FFFFFF0]), rng.choice([0, 3, 9, 50, -1])) for _ in w] for w in lists] for g in (1, 2)}
    stride = total + 4
    ref_start, ref_end = poisoned_words(2 * stride), poisoned_words(2 * stride)
    for r, g in enumerate((1, 2)):
        flat = [x for w in wild[g] for x in w]
        ref_start[r * stride:r * stride + total] = torch.tensor([a for a, _ in flat], dtype=torch.int32)
        ref_end[r * stride:r * stride + total] = torch.tensor([b for _, b in flat], dtype=torch.int32)
    clamp = lambda it, a, b: (-1, -1) if a == -1 else (min(a & NONE, len(it)), min(max(b & NONE, min(a & NONE, len(it))), len(it)))
    clamped = {g: [[clamp(it, a, b) for a, b in w] for it, w in zip(items, wild[g])] for g in (1, 2)}
    want = column([splice_template(it, w, {g: clamped[g][k] for g in (1, 2)}, parse_py(tpl.repl)) for k, (it, w) in enumerate(zip(items, lists))])
    length, pos = poisoned_words(n + 1), poisoned_words(total + 1)
    rr._check(L.rrx_replace_template_sizes(0, ptr(doff), n, 1, ptr(first), ptr(start), ptr(end), tpl._h, ptr(ref_start), ptr(ref_end), stride, ptr(length), ptr(pos), s))
    out_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    out_off[1:] = torch.cumsum(length[:n].to(torch.int64) & 0xFFFFFFFF, dim=0)
    g = Guarded(int(out_off[-1]), mis=1)
    rr._check(L.rrx_replace_template_fill(0, ptr(dev), ptr(doff), n, 1, ptr(first), ptr(start), ptr(end), ptr(pos), tpl._h, ptr(ref_start), ptr(ref_end), stride,
                                          ptr(out_off), ptr(g.d_out), s))
    torch.cuda.synchronize()
    assert_column(g.written("wild planes"), out_off.cpu().numpy(), want[0], want[1], "wild planes")


def test_tables_in_global_memory():
    """RRX_ENGINE_DFA_GLOBAL forces the list kernel's tables into HBM/L2."""
    p, ngroups, items, lists, spans = next(x for x in reference_templates() if x[0] == DATE)
    groups = [rr.RGroup(p, g, rr.ENGINE_DFA_GLOBAL) for g in (1, 2, 3)]
    dev, doff = to_dev(*pack(items, 1, lead=7))
    for repl in (rb"\3-\1-\2", rb"\2\2"):
        outs = expected_items(items, lists, spans, repl)
        generic(groups, repl, dev, doff, 1, column(outs), ("global form", repl), first0=2, extra_stride=1, want_spans=spans)
        one_call(groups, repl, dev, doff, 1, column(outs), ("global form, one call", repl))


def test_a_side_stream_and_a_captured_graph(handles):
    p, ngroups, items, lists, spans = next(x for x in reference_templates() if x[0] == DATE)
    groups, repl = handles[p], rb"\3-\1-\2"
    items, n = list(items), len(items)
    text, offs = pack(items, 1, lead=1)
    dev, doff = to_dev(text, offs)
    want = column(expected_items(items, lists, spans, repl))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    out, off = rr.replace_groups_longest_extents(groups, repl, dev, doff, trim=1, stream=side)      # (the warm-up: tables and template are uploaded here)
    first, start, end = groups[0].regex.search_all_longest_extents_fused(dev, doff, trim=1, stream=side)
    planes = [g.spans_list_extents(dev, doff, first, start, end, trim=1, stream=side) for g in groups]
    out2, off2 = rr.replace_template(dev, doff, first, start, end, rr.Template(repl), torch.cat([pl[0] for pl in planes]), torch.cat([pl[1] for pl in planes]),
                                     trim=1, stream=side)
    side.synchronize()
    assert_column(out.cpu().numpy(), off.cpu().numpy(), want[0], want[1], "side stream, one call")
    assert_column(out2.cpu().numpy(), off2.cpu().numpy(), want[0], want[1], "side stream, generic")
    # list spans, sizes, the prefix and fill captured once (nothing is allocated by the entries, uploaded or read back inside),
    # replayed on refilled inputs: the items in another order, their lists with them
    L, tpl = rr._L, rr.Template(repl)
    rr.replace_template(dev, doff, first, start, end, tpl, torch.cat([pl[0] for pl in planes]), torch.cat([pl[1] for pl in planes]), trim=1, stream=side)
    side.synchronize()
    total = int(first[-1])
    words = L.rrx_search_all_longest_marks_words(len(text), n)
    marks = poisoned_words(words)
    ref_start, ref_end = poisoned_words(3 * total), poisoned_words(3 * total)
    length, pos = poisoned_words(n), poisoned_words(total)
    out_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    g = Guarded(len(want[0]), mis=2)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            s = rr._stream_ptr(side)
            for r, grp in enumerate(groups):
                rr._check(L.rrx_group_spans_list_extents(grp._h, 0, ptr(dev), ptr(doff), n, 1, ptr(first), ptr(start), ptr(end), ptr(marks), words,
                                                         ptr(ref_start[r * total:]), ptr(ref_end[r * total:]), s))
            rr._check(L.rrx_replace_template_sizes(0, ptr(doff), n, 1, ptr(first), ptr(start), ptr(end), tpl._h, ptr(ref_start), ptr(ref_end), total, ptr(length),
                                                   ptr(pos), s))
            torch.cumsum(length.to(torch.int64), dim=0, out=out_off[1:])
            rr._check(L.rrx_replace_template_fill(0, ptr(dev), ptr(doff), n, 1, ptr(first), ptr(start), ptr(end), ptr(pos), tpl._h, ptr(ref_start), ptr(ref_end),
                                                  total, ptr(out_off), ptr(g.d_out), s))
    torch.cuda.current_stream().wait_stream(side)
    for round_, order in enumerate((list(range(n)), list(reversed(range(n))))):
        text2, offs2 = pack([items[k] for k in order], 1, lead=1)
        assert len(text2) == len(text)
        dev.copy_(torch.from_numpy(text2))
        doff.copy_(torch.from_numpy(offs2))
        f2, s2, e2 = groups[0].regex.search_all_longest_extents_fused(dev, doff, trim=1)
        first.copy_(f2)
        start.copy_(s2)
        end.copy_(e2)
        for t in (marks, ref_start, ref_end, length, pos):
            t.fill_(WORD_POISON)
        g.buf.fill_(0x5A)
        graph.replay()
        torch.cuda.synchronize()
        want2 = column(expected_items([items[k] for k in order], [lists[k] for k in order], {q: [spans[q][k] for k in order] for q in spans}, repl))
        assert_column(g.written(("replay", round_)), out_off.cpu().numpy(), want2[0], want2[1], ("replay", round_))


def test_the_cap_protocol_and_degenerate_batches(handles):
    L, s = rr._L, rr._stream_ptr(None)
    p, ngroups, items, lists, spans = next(x for x in reference_templates() if x[0] == DATE)
    groups, repl = handles[p], rb"<\2\2\0>"
    tpl, h = rr.Template(repl), rr._group_handles(handles[p])
    dev, doff = to_dev(*pack(items, 1, lead=1))
    handle = rr.Items(dev, doff, trim=1)
    n = len(items)
    want = column(expected_items(items, lists, spans, repl))
    total = len(want[0])
    assert total > 2 * n
    for indexed in (False, True):
        for cap in (total - 1, 0, total, total + 5):
            g, tot = Guarded(total), C.c_size_t(99)
            out_off = torch.full((n + 2,), -7, dtype=torch.int64, device="cuda")
            d_out = ptr(g.d_out) if cap else None
            if indexed:
                rr._check(L.rrx_replace_groups_longest_items(h, 3, tpl._h, handle._h, ptr(out_off), d_out, cap, C.byref(tot), s))
            else:
                rr._check(L.rrx_replace_groups_longest_extents(h, 3, tpl._h, 0, ptr(dev), ptr(doff), n, 1, ptr(out_off), d_out, cap, C.byref(tot), s))
            torch.cuda.synchronize()
            assert tot.value == total and int(out_off[n + 1]) == -7 and np.array_equal(out_off[:n + 1].cpu().numpy(), want[1]), (indexed, cap, "d_out_off is complete either way")
            if cap < total:
                g.untouched((indexed, cap))
            else:
                assert np.array_equal(g.written((indexed, cap)), want[0]), (indexed, cap)
    assert L.rrx_replace_groups_longest_extents(h, 3, tpl._h, 0, ptr(dev), ptr(doff), n, 1, ptr(out_off), None, 5, C.byref(tot), s) == 2      # RRX_ERR_ARG: cap > 0 and no d_out
    # nitems == 0: the generic entries write nothing, the one-call forms d_out_off[0] = 0
    nothing = torch.empty(0, dtype=torch.uint8, device="cuda")
    zero = torch.zeros(1, dtype=torch.int64, device="cuda")
    g, w = Guarded(8), poisoned_words(4)
    assert L.rrx_group_spans_list_extents(groups[0]._h, 0, None, ptr(zero), 0, 0, ptr(zero), ptr(w), ptr(w), ptr(w), 4, ptr(w), ptr(w), s) == 0
    assert L.rrx_replace_template_sizes(0, ptr(zero), 0, 0, ptr(zero), ptr(w), ptr(w), tpl._h, ptr(w), ptr(w), 4, ptr(w), ptr(w), s) == 0
    assert L.rrx_replace_template_fill(0, None, ptr(zero), 0, 0, ptr(zero), ptr(w), ptr(w), ptr(w), tpl._h, ptr(w), ptr(w), 4, ptr(zero), ptr(g.d_out), s) == 0
    torch.cuda.synchronize()
    g.untouched("empty batch")
    assert bool((w == WORD_POISON).all())
    empty = (np.empty(0, dtype=np.uint8), np.zeros(1, dtype=np.int64))
    one_call(groups, repl, nothing, zero, 0, empty, "empty batch")
    one_call(groups, repl, nothing, zero, 0, empty, "empty batch, indexed", handle=rr.Items(nothing, zero))
    out, off = rr.replace_groups_longest_extents(groups, repl, nothing, zero)
    assert out.numel() == 0 and off.tolist() == [0]
    # a batch of empty items; items without any match: copied
    off0 = torch.zeros(71, dtype=torch.int64, device="cuda")
    one_call(groups, repl, nothing, off0, 0, column([b""] * 70), "empty items")
    generic(groups, repl, nothing, off0, 0, column([b""] * 70), "empty items, generic")
    plain = [b"no date", b"", b"1/2"] * 30
    dev2, doff2 = to_dev(*pack(plain, 1, lead=3))
    one_call(groups, repl, dev2, doff2, 1, column(plain), "no match anywhere")
    generic(groups, repl, dev2, doff2, 1, column(plain), "no match anywhere, generic", first0=4, extra_stride=2)
    # the empty language copies the items (list spans: a fill over no slot), the empty template deletes the matches
    void = [rr.RGroup("a([])b", 1)]
    one_call(void, rb"<\1>", dev, doff, 1, column(list(items)), "the empty language")
    generic(void, rb"<\1>", dev, doff, 1, column(list(items)), "the empty language, generic")
    first, start, end = groups[0].regex.search_all_longest_extents_fused(dev, doff, trim=1)
    got = void[0].spans_list_extents(dev, doff, first, start, end, trim=1)
    assert bool((got[0] == -1).all()) and bool((got[1] == -1).all()) and got[0].numel() == int(first[-1]) > 0


def test_an_output_item_of_2_30_bytes_is_refused():
    """test_replace_items_gpu's case on the template's sizes kernel: one item of 65536 b"a", (a) matching every byte, a template that
    is a literal of 16383 bytes (2^30 - 65536 output bytes: accepted) and of 16384 (exactly 2^30: refused, the total left 0), cap = 0
    and no d_out; the flag is the call's own: the next call goes through."""
    L, s = rr._L, rr._stream_ptr(None)
    groups = [rr.RGroup("(a)", 1)]
    h = rr._group_handles(groups)
    dev, doff = to_dev(*pack([b"a" * 65536], 0))

    def call(repl):
        tpl, tot, out_off = rr.Template(repl), C.c_size_t(99), torch.full((2,), -7, dtype=torch.int64, device="cuda")
        rc = L.rrx_replace_groups_longest_extents(h, 1, tpl._h, 0, ptr(dev), ptr(doff), 1, 0, ptr(out_off), None, 0, C.byref(tot), s)
        torch.cuda.synchronize()
        return rc, tot.value, out_off.cpu().tolist()

    assert call(b"r" * 16383) == (0, 65536 * 16383, [0, 65536 * 16383])
    rc, total, _ = call(b"r" * 16384)
    assert (rc, total) == (4, 0)                                                           # RRX_ERR_UNSUPPORTED
    assert L.rrx_last_error() == (b"an output item of 2^30 bytes or more: use rrx_search_all_longest_extents, rrx_group_spans_list_extents and the two "
                                  b"passes rrx_replace_template_sizes / _fill")
    assert call(b"r") == (0, 65536, [0, 65536])
