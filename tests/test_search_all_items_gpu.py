"""rrx_search_all_extents* / rrx_search_all_items* on the device: every match of every item, match k + 1 searched in the rest of the
item behind match k.  Against the oracle's brute force on short items (the CPU test's patterns, items and reference), re.finditer
with the lazy spelling on patterns for which it names the same matches (test_search_all_items_lowering checks that), and
rrx_search_all element for element on '\\n' text viewed as items."""
import ctypes as C
import random
import re

import numpy as np
import pytest

import roaringregex_amd as rr
from contains_cases import EXPLODING, short_line_patterns
from patterns import EMAIL, K1000_CONTAINS, U2
from test_contains_items_lowering import NEWLINE_PATTERNS, short_items
from test_search_all_items_lowering import lazy_all, want_for
from test_search_items_gpu import POOL, pack, pooled_batch, to_dev
from test_search_items_lowering import GLOBAL_AUTO, NITEMS, plain_table_bytes

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
MAX_BLOCKS_ITEMS = 1024 * 1024                      # kernels_search_all_items.hip: 1024 workgroups of 1024 lanes, then the grid strides


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"


def csr(want):
    """[[(start, end)]] per item -> (count[n] int32, first[n + 1] int64, pairs[total, 2] int32), read-only."""
    count = np.array([len(w) for w in want], dtype=np.int32)
    first = np.concatenate([[0], np.cumsum(count, dtype=np.int64)]).astype(np.int64)
    pairs = np.array([x for w in want for x in w], dtype=np.int32).reshape(-1, 2)
    for a in (count, first, pairs):
        a.setflags(write=False)
    return count, first, pairs


@pytest.fixture(scope="module")
def reference():
    """[(pattern, items, (count, first, pairs))]: the CPU test's patterns, items (same seed) and brute force - computed once."""
    rng = random.Random(1901)
    out = []
    for p in short_line_patterns() + NEWLINE_PATTERNS:
        items = short_items(rng, p, NITEMS)
        out.append((p, items, csr(want_for(p, items))))
    return out


def assert_csr(got, want, what):
    """got: (count or None, first, start, end) device tensors; first has n entries (two passes) or n + 1 (one call)."""
    count, first, pairs = want
    g_count, g_first, g_start, g_end = got
    n, total = len(count), len(pairs)
    if g_count is not None:
        assert np.array_equal(g_count.cpu().numpy(), count), (what, "count")
        assert g_first.numel() == n
    else:
        assert g_first.numel() == n + 1 and int(g_first[-1]) == total, (what, "first[-1] is the total")
    assert np.array_equal(g_first.cpu().numpy(), first[:g_first.numel()]), (what, "first")
    assert g_start.numel() == total and g_end.numel() == total, (what, g_start.numel(), total)
    got_pairs = torch.stack([g_start, g_end], dim=1).cpu().numpy()
    bad = np.nonzero((got_pairs != pairs).any(axis=1))[0]
    assert bad.size == 0, (what, "first bad slot", int(bad[0]), "item", int(np.searchsorted(first, bad[0], side="right")) - 1,
                           got_pairs[bad[0]].tolist(), pairs[bad[0]].tolist())


def run_all_forms(r, dev, doff, trim, want, what, handle=None, caps=(None, 1, 0)):
    """count + fill, then the one-call form at every cap - on the offsets, or on an indexed batch."""
    if handle is None:
        assert_csr(r.search_all_extents(dev, doff, trim=trim), want, (what, "two passes"))
        for cap in caps:
            assert_csr((None,) + r.search_all_extents_fused(dev, doff, trim=trim, cap=cap), want, (what, "one call, cap", cap))
    else:
        assert_csr(r.search_all_items(handle), want, (what, "indexed, two passes"))
        for cap in caps:
            assert_csr((None,) + r.search_all_items_fused(handle, cap=cap), want, (what, "indexed, one call, cap", cap))


def test_short_items_against_the_brute_force(reference):
    for p, items, want in reference:
        r = rr.RRegex(p)
        for trim in (0, 1):
            dev, doff = to_dev(*pack(items, trim, lead=trim * 3, seed=len(items) + trim))
            run_all_forms(r, dev, doff, trim, want, (p[:30], "trim", trim))
            run_all_forms(r, dev, doff, trim, want, (p[:30], "trim", trim), handle=rr.Items(dev, doff, trim=trim))


def finditer_csr(p, pool, idx):
    """The CSR arrays of a batch drawn from `pool` by `idx`, from re.finditer per pool item (numpy: the batch may pass a million)."""
    per = [lazy_all(p, it) for it in pool]
    width = max(len(w) for w in per)
    pc = np.array([len(w) for w in per], dtype=np.int32)
    ps = np.zeros((len(pool), width, 2), dtype=np.int32)
    for k, w in enumerate(per):
        ps[k, :len(w)] = np.array(w, dtype=np.int32).reshape(-1, 2)
    count = pc[idx]
    first = np.concatenate([[0], np.cumsum(count, dtype=np.int64)]).astype(np.int64)
    item_of_slot = np.repeat(np.arange(len(idx)), count)
    rank = np.arange(int(first[-1])) - first[item_of_slot]
    return count, first, ps[idx[item_of_slot], rank]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130, 4097, MAX_BLOCKS_ITEMS + 65])
def test_batch_sizes(n):
    """Wave edges, more than one workgroup and more items than one pass of the grid holds; the offsets do not begin at 0, the text
    tensor ends with the last item, and trim 3 is larger than some items (region = item + ';')."""
    p, trim, lead = "ab+c", 3, 16
    r = rr.RRegex(p)
    text, off, idx = pooled_batch(n, 40 + n % 7, trim, lead)
    assert off[0] == lead != 0 and off[-1] == len(text)
    trimmed = [(it + b";")[:max(len(it) + 1 - trim, 0)] for it in POOL]
    assert any(len(it) + 1 < trim for it in POOL)
    want = finditer_csr(p, trimmed, idx)
    dev, doff = to_dev(text, off)
    assert dev.untyped_storage().nbytes() == int(off[-1])
    run_all_forms(r, dev, doff, trim, want, ("batch", n), caps=(None,) if n > 4097 else (None, 1, 0))
    assert n < 4097 or 0 < int((want[0] > 0).sum()) < n


def test_every_alignment_of_item_start_match_ends_starts_and_restarts():
    """40-byte items with two or three matches of ab+c, one of them at every offset it has room for; each item at all 16 alignments
    of its first byte (items of 41 bytes with their separator: 16 consecutive copies walk through the residues), and the whole
    buffer off 16-byte alignment as well."""
    p = "ab+c"
    items = []
    for at in range(3, 38):                         # "abc" in front, a moving "abc", and "abc" at the end where it still fits
        it = bytearray(b"z" * 40)
        it[0:3] = b"abc"
        if at + 3 <= 37:
            it[37:40] = b"abc"
        it[at:at + 3] = b"abc"
        items += [bytes(it)] * 16
    long_needle = b"a" + b"b" * 19 + b"c"           # (its walk back crosses a 16-byte boundary and ends at a floor)
    for at in range(0, 17):
        it = bytearray(b"z" * 40)
        it[at:at + 3] = b"abc"
        it[19:40] = long_needle
        items += [bytes(it)] * 16
    want_lists = [lazy_all(p, it) for it in items]
    assert all(len(it) == 40 for it in items) and {len(w) for w in want_lists} == {2, 3}
    want = csr(want_lists)
    r = rr.RRegex(p)
    for lead in (0, 3):
        text, offs = pack(items, 1, lead)
        starts, ends, restarts = set(), set(), set()
        for o, w in zip(offs[:-1], want_lists):
            starts |= {(int(o) + s) % 16 for s, _ in w}
            ends |= {(int(o) + e) % 16 for _, e in w}
            restarts |= {(int(o) + e) % 16 for _, e in w[:-1]}          # where the search of a later match begins
        assert len({int(o) % 16 for o in offs[:-1]}) == 16 and len(starts) == 16 and len(ends) == 16 and len(restarts) == 16
        dev, doff = to_dev(text, offs)
        assert dev.data_ptr() % 16 == 0
        run_all_forms(r, dev, doff, 1, want, ("alignment", lead), caps=(None,))
        sliced = torch.cat([torch.zeros(5, dtype=torch.uint8, device="cuda"), dev])[5:]
        assert sliced.data_ptr() % 16 == 5
        run_all_forms(r, sliced, doff, 1, want, ("alignment, sliced", lead), caps=(None,))


def re_all_brute_force(rx, item):
    """The issue's rule with Python's fullmatch (patterns whose syntax the dialects share, none of which accepts "")."""
    c = re.compile(rx)
    out, p = [], 0
    while p < len(item):
        hit = next(((s, e) for e in range(p + 1, len(item) + 1) for s in range(p, e) if c.fullmatch(item, s, e)), None)
        if hit is None:
            break
        out.append(hit)
        p = hit[1]
    return out


def test_long_and_dense_items():
    """30000 matches in one item, 100000 one-byte matches, a walk back over 30 KB, sparse 5 ... 100 KB items with their matches
    near the end - on the LDS tables, with both tables forced into HBM/L2, and on a pattern whose tables pass 64 KiB by themselves."""
    rng = random.Random(31)
    fill = b"xy zb" * 20001                                         # (no 'a': neither pattern matches inside it)
    for p, needles in (("ab+c", [b"abc", b"abbbbbc", b"a" + b"b" * 30000 + b"c"]), ("a{1,300}", [b"a", b"a" * 1000])):
        items = [b"abc" * 30000] if p == "ab+c" else [b"a" * 100000]
        for k in range(45):
            n = rng.choice([5000, 5001, 20000, 65536, 100000])
            needle = needles[k % len(needles)]
            tail = rng.choice([0, 1, 15, 16, 17, 300])
            body = needle + fill[:rng.choice([0, 1, 14, 40])] + needles[0] + fill[:tail]
            items.append(fill[:max(n - len(body), 0)] + body if k % 9 else fill[:n])      # one item in nine has no match
        want_lists = [lazy_all(p, it) for it in items]
        counts = [len(w) for w in want_lists]
        assert counts[0] == (30000 if p == "ab+c" else 100000) and 0 < sum(c == 0 for c in counts) < len(items)
        assert max(e for w in want_lists for _, e in w) > 99000
        if p == "ab+c":
            assert max(e - s for w in want_lists for s, e in w) == 30002
        short = [it[-22:] for it in items[1:]]                      # the last 22 bytes: the brute force and finditer agree
        assert want_for(p, short) == [lazy_all(p, it) for it in short]
        want = csr(want_lists)
        for engine in (rr.ENGINE_AUTO, rr.ENGINE_DFA_GLOBAL):
            r = rr.RRegex(p, engine)
            for trim, lead in ((0, 0), (1, 7)):
                dev, doff = to_dev(*pack(items, trim, lead, seed=trim))
                run_all_forms(r, dev, doff, trim, want, (p, "long", engine, trim), caps=(None,))
    r = rr.RRegex(GLOBAL_AUTO)
    assert plain_table_bytes(r.program(rr.PROGRAM_SEARCH_FWD)) + plain_table_bytes(r.program(rr.PROGRAM_SEARCH_REV)) > 65536
    items = ["".join(rng.choice("aaabbbx") for _ in range(rng.choice([0, 5, 13, 14, 15, 31, 32, 33, 60]))).encode() for _ in range(150)]
    w = b"a" + b"b" * 12 + b"x"                                     # (a shortest match; random items hardly ever hold two)
    items += [w, w * 3, b"x" * 20 + b"ab" * 20 + b"x", b"ab" * 7 + b"x" + b"ba" * 7 + b"xx", b"b" * 7 + b"a" + b"ab" * 6 + b"x" + w,
              b"x" + (b"a" * 13 + b"x") * 2 + b"b", w + b"bxab" + b"a" * 14 + b"x" + w]
    want_lists = [re_all_brute_force(GLOBAL_AUTO.encode(), it) for it in items]
    short = [k for k, it in enumerate(items) if len(it) <= 22]
    assert want_for(GLOBAL_AUTO, [items[k] for k in short]) == [want_lists[k] for k in short]      # (re and the oracle agree where both can tell)
    assert sum(len(w) >= 2 for w in want_lists) >= 3 and 20 < sum(len(w) >= 1 for w in want_lists) < len(items)
    for trim, lead in ((0, 0), (1, 9)):
        dev, doff = to_dev(*pack(items, trim, lead))
        run_all_forms(r, dev, doff, trim, csr(want_lists), ("AUTO, tables beyond the LDS budget", trim))


@pytest.mark.parametrize("kind", ["url", "email", "kwlog"])
def test_search_all_extents_equals_search_all(kind):
    """16 MiB of '\\n' text viewed as items - offsets = the line starts, trim 1: count, first, start and end of rrx_search_all*."""
    import synth
    pattern = {"url": U2, "email": EMAIL, "kwlog": K1000_CONTAINS}[kind]
    host = synth.corpus(kind, 6, 16 << 20)
    host = host[:int(np.nonzero(host == 10)[0][-1]) + 1]                 # (whole lines: every item has its separator)
    r = rr.RRegex(pattern)
    dev = torch.from_numpy(host).cuda()
    corpus = rr.Corpus(dev)
    wc, wf, ws, we = r.search_all(corpus)
    n = corpus.num_lines
    off = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.nonzero(dev == 10).flatten() + 1]).contiguous()
    assert off.numel() == n + 1 and ws.numel() > 0
    for what, got in (("extents", r.search_all_extents(dev, off, trim=1)), ("items", r.search_all_items(rr.Items(dev, off, trim=1)))):
        for name, g, w in zip(("count", "first", "start", "end"), got, (wc, wf, ws, we)):
            assert g.shape == w.shape and torch.equal(g, w), (kind, what, name, int(torch.nonzero(g != w)[0]) if g.shape == w.shape else g.shape)
    gf, gs, ge = r.search_all_extents_fused(dev, off, trim=1)
    assert torch.equal(gf[:-1], wf) and int(gf[-1]) == ws.numel() and torch.equal(gs, ws) and torch.equal(ge, we), (kind, "one call")


def poisoned(n):
    return torch.full((n,), POISON, dtype=torch.int32, device="cuda")


def test_edge_patterns_and_output_buffers():
    rng = random.Random(33)
    items = short_items(rng, "ab+c", 131) + [b"abcabbc;abc", b"abc" * 7] + [b"z" * k + b"abbc" * 5 for k in range(3)]
    n = len(items)
    text, offs = pack(items, 1, lead=2)
    dev, doff = to_dev(text, offs)
    handle = rr.Items(dev, doff, trim=1)
    L, stream = rr._L, rr._stream_ptr(None)
    empty_lang = [[] for _ in items]
    for p, want_lists in (("ab+c", want_for("ab+c", items)), ("a*", [[(k, k) for k in range(len(it) + 1)] for it in items]), ("[]", empty_lang)):
        r = rr.RRegex(p)
        count, first, pairs = csr(want_lists)
        total = len(pairs)
        assert p == "[]" or total > n // 4
        d_first = torch.from_numpy(first.copy()).cuda()
        for indexed in (False, True):
            # _count writes exactly nitems words, _fill exactly `total` slots
            cnt, st, en = poisoned(n + 1), poisoned(total + 1), poisoned(total + 1)
            if indexed:
                rr._check(L.rrx_search_all_items_count(r._h, handle._h, cnt.data_ptr(), stream))
                rr._check(L.rrx_search_all_items_fill(r._h, handle._h, d_first.data_ptr(), st.data_ptr(), en.data_ptr(), stream))
            else:
                rr._check(L.rrx_search_all_extents_count(r._h, 0, dev.data_ptr(), doff.data_ptr(), n, 1, cnt.data_ptr(), stream))
                rr._check(L.rrx_search_all_extents_fill(r._h, 0, dev.data_ptr(), doff.data_ptr(), n, 1, d_first.data_ptr(), st.data_ptr(), en.data_ptr(), stream))
            torch.cuda.synchronize()
            assert int(cnt[n]) == POISON and int(st[total]) == POISON and int(en[total]) == POISON, (p, indexed, "a word behind the results was written")
            assert_csr((cnt[:n], d_first[:n], st[:total], en[:total]), (count, first, pairs), (p, indexed, "poisoned"))
            # the one-call form with cap < total: d_first complete, slots >= cap untouched
            for cap in (total // 2, 0):
                fst, st, en, tot = torch.full((n + 2,), POISON, dtype=torch.int64, device="cuda"), poisoned(total + 1), poisoned(total + 1), C.c_size_t(99)
                if indexed:
                    rr._check(L.rrx_search_all_items(r._h, handle._h, fst.data_ptr(), st.data_ptr(), en.data_ptr(), cap, C.byref(tot), stream))
                else:
                    rr._check(L.rrx_search_all_extents(r._h, 0, dev.data_ptr(), doff.data_ptr(), n, 1, fst.data_ptr(), st.data_ptr(), en.data_ptr(), cap,
                                                       C.byref(tot), stream))
                torch.cuda.synchronize()
                assert tot.value == total and int(fst[n + 1]) == POISON and np.array_equal(fst[:n + 1].cpu().numpy(), first), (p, indexed, cap)
                assert (st[cap:] == POISON).all() and (en[cap:] == POISON).all(), (p, indexed, cap, "a slot >= cap was written")
                assert np.array_equal(torch.stack([st[:cap], en[:cap]], dim=1).cpu().numpy(), pairs[:cap]), (p, indexed, cap)
    # cap == 0 needs no match arrays
    r, tot = rr.RRegex("ab+c"), C.c_size_t(0)
    fst = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    rr._check(L.rrx_search_all_extents(r._h, 0, dev.data_ptr(), doff.data_ptr(), n, 1, fst.data_ptr(), None, None, 0, C.byref(tot), stream))
    assert tot.value == int(fst[-1]) == len(csr(want_for("ab+c", items))[2])
    assert L.rrx_search_all_extents(r._h, 0, dev.data_ptr(), doff.data_ptr(), n, 1, fst.data_ptr(), None, None, 5, C.byref(tot), stream) == 2      # RRX_ERR_ARG
    # all-empty items: nothing but offsets; an empty batch: first[0] = 0
    nothing = torch.empty(0, dtype=torch.uint8, device="cuda")
    zero = torch.zeros(1, dtype=torch.int64, device="cuda")
    off0 = torch.zeros(71, dtype=torch.int64, device="cuda")
    run_all_forms(r, nothing, off0, 0, csr([[]] * 70), "all-empty items")
    run_all_forms(rr.RRegex("a*"), nothing, off0, 0, csr([[(0, 0)]] * 70), "all-empty items, nullable")
    run_all_forms(rr.RRegex("a*"), dev, doff, 40, csr([[(0, 0)]] * n), "a trim larger than every item, nullable")
    for rx in (r, rr.RRegex("a*")):
        run_all_forms(rx, nothing, zero, 0, csr([]), "empty batch")
        run_all_forms(rx, nothing, zero, 0, csr([]), "empty batch", handle=rr.Items(nothing, zero))
    bad = rr.RRegex(EXPLODING)
    for call in (lambda: bad.search_all_extents(dev, doff, trim=1), lambda: bad.search_all_items(handle), lambda: bad.search_all_extents_fused(dev, doff, trim=1),
                 lambda: bad.search_all_items_fused(handle), lambda: bad.search_all_extents(nothing, zero), lambda: bad.search_all_items(rr.Items(nothing, zero)),
                 lambda: bad.search_all_extents_fused(nothing, zero), lambda: bad.search_all_items_fused(rr.Items(nothing, zero))):
        with pytest.raises(rr.RRegexError, match="determinise"):
            call()
    st, no_items = poisoned(4), rr.Items(nothing, zero)
    for fn, args in ((L.rrx_search_all_items_count, (st.data_ptr(),)), (L.rrx_search_all_items_fill, (fst.data_ptr(), st.data_ptr(), st.data_ptr()))):
        assert fn(bad._h, no_items._h, *args, stream) == 4                                # RRX_ERR_UNSUPPORTED, for an empty batch too


def test_count_and_fill_on_a_side_stream_and_in_one_captured_graph(reference):
    p, items, _ = next(x for x in reference if x[0] == EMAIL)
    want_lists = want_for(p, items)
    want = csr(want_lists)
    n, total = len(items), len(want[2])
    assert total > n // 4
    r = rr.RRegex(p)
    text, offs = pack(items, 1, lead=1)
    dev, doff = to_dev(text, offs)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    got = r.search_all_extents(dev, doff, trim=1, stream=side)
    side.synchronize()
    assert_csr(got, want, "side stream")
    # count, the prefix and fill captured into one graph (the tables are up: nothing is uploaded inside the capture), replayed on
    # refilled inputs: the same items in another order have the same total
    cnt, st, en = poisoned(n), poisoned(total), poisoned(total)
    inclusive = torch.zeros(n, dtype=torch.int64, device="cuda")
    first = torch.zeros(n, dtype=torch.int64, device="cuda")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            s = rr._stream_ptr(side)
            rr._check(rr._L.rrx_search_all_extents_count(r._h, 0, dev.data_ptr(), doff.data_ptr(), n, 1, cnt.data_ptr(), s))
            torch.cumsum(cnt, dim=0, dtype=torch.int64, out=inclusive)
            torch.sub(inclusive, cnt, out=first)
            rr._check(rr._L.rrx_search_all_extents_fill(r._h, 0, dev.data_ptr(), doff.data_ptr(), n, 1, first.data_ptr(), st.data_ptr(), en.data_ptr(), s))
    torch.cuda.current_stream().wait_stream(side)
    for round_, order in enumerate((list(range(n)), list(reversed(range(n))))):
        shuffled = [items[k] for k in order]
        text2, offs2 = pack(shuffled, 1, lead=1)
        assert len(text2) == len(text)
        dev.copy_(torch.from_numpy(text2))
        doff.copy_(torch.from_numpy(offs2))
        for t in (cnt, st, en):
            t.fill_(POISON)
        g.replay()
        torch.cuda.synchronize()
        want2 = csr([want_lists[k] for k in order])
        assert_csr((cnt, first, st, en), want2, ("replay", round_))
        assert_csr(r.search_all_extents(dev, doff, trim=1), want2, ("direct call", round_))
