"""rrx_multi_contains_extents / _items, rrx_multi_counts and rrx_multi_plane on the device.  The reference is the existing
single-pattern entry, RRegex.contains_extents_bits per member on the SAME tensors (bit k of mask i = bit i of member k's bitmap),
and on the short items of multi_cases the CPU brute force as well."""
import random

import numpy as np
import pytest

import roaringregex_amd as rr
from contains_cases import unpack
from multi_cases import SETS, items_of, pack_items, want_masks
from test_contains_items_lowering import oracle_for, shortest_accepted

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
GUARD = 8                                               # words behind nitems that no launch may touch
_regex = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"


def member(p):
    if p not in _regex:
        _regex[p] = rr.RRegex(p)
    return _regex[p]


def to_dev(text, offs):
    d = torch.from_numpy(text).cuda() if len(text) else torch.empty(0, dtype=torch.uint8, device="cuda")
    return d, torch.from_numpy(offs).cuda()


def member_masks(pats, dev, doff, trim):
    """uint32 per item from the single-pattern entries: bit k = RRegex(pats[k]).contains_extents_bits, one call per distinct pattern."""
    n = doff.numel() - 1
    cols, m = {}, np.zeros(n, dtype=np.uint32)
    for k, p in enumerate(pats):
        if p not in cols:
            cols[p] = unpack(member(p).contains_extents_bits(dev, doff, trim=trim).cpu().numpy(), n).astype(np.uint32) if n else np.zeros(0, np.uint32)
        m |= cols[p] << np.uint32(k)
    return m


def guarded(n):
    return torch.full((n + GUARD,), POISON, dtype=torch.int32, device="cuda")


def run(m, dev, doff, trim=0, handle=None, stream=None):
    """The masks as uint32, through a poisoned buffer with guard words behind nitems: every word written, none beyond."""
    n = doff.numel() - 1
    buf = guarded(n)
    out = m.contains_items(handle, out=buf, stream=stream) if handle is not None else m.contains_extents(dev, doff, trim=trim, out=buf, stream=stream)
    torch.cuda.synchronize()
    assert out.numel() == n and out.data_ptr() == buf.data_ptr()
    assert (buf[n:] == POISON).all(), "words behind the masks were written"
    return out.cpu().numpy().view(np.uint32)


def same(got, want, what, items=None):
    assert got.shape == want.shape
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (what, int(bad[0]), hex(int(got[bad[0]])), hex(int(want[bad[0]])), None if items is None else items[bad[0]])


def builds(pats):
    """The one-group-if-it-fits build, a build forced into three groups at least (the OR launches), the forced global build."""
    cut = rr.RMulti(pats, max_rows=8)
    out = [("default", rr.RMulti(pats)), ("global", rr.RMulti(pats, engine=rr.ENGINE_DFA_GLOBAL))]
    if len(pats) >= 5:
        assert cut.groups >= 3, cut.groups
    return out + [("cut", cut)]


@pytest.mark.parametrize("name", list(SETS))
def test_short_items_against_the_brute_force_and_the_members(name):
    pats, items, want = SETS[name], items_of(name), want_masks(name)
    ms = builds(pats)
    for trim in (0, 1):
        text, offs = pack_items(items, trim=trim, lead=3, sep=b"b")       # (a separator that would complete "ab", were it read)
        dev, doff = to_dev(text, offs)
        same(member_masks(pats, dev, doff, trim), want, (name, trim, "the members themselves"), items)
        handle = rr.Items(dev, doff, trim=trim)
        for what, m in ms:
            same(run(m, dev, doff, trim), want, (name, trim, what, "raw offsets"), items)
            same(run(m, dev, doff, handle=handle), want, (name, trim, what, "rr.Items"), items)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 5000])
def test_batch_sizes(n):
    base = items_of("twelve")
    items = [base[(7 * i) % len(base)] for i in range(n)]
    dev, doff = to_dev(*pack_items(items))
    want = member_masks(SETS["twelve"], dev, doff, 0)
    assert n < 64 or want.any()
    for what, m in builds(SETS["twelve"]):
        same(run(m, dev, doff), want, (n, what), items)


def geometry_items(rng):
    """Every residue of the item's start mod 16 with every length 0 .. 40: a filler item in front of each moves the start there."""
    alphabet, needles = b"abck01.d@yz\n", [b"abbc", b"k100", b"1.5", b"aab", b"a@b", b"\xffab\x00c"]
    items, at, seen = [], 0, set()
    for length in range(41):
        for residue in range(16):
            fill = (residue - at) % 16
            items.append(bytes(rng.choice(alphabet) for _ in range(fill)))
            at += fill
            body = bytearray(rng.choice(alphabet) for _ in range(length))
            if length >= 6 and rng.random() < 0.5:
                nd = rng.choice(needles)
                p = rng.randrange(length - len(nd) + 1)
                body[p:p + len(nd)] = nd
            assert at % 16 == residue
            seen.add((residue, length))
            items.append(bytes(body))
            at += length
    assert len(seen) == 16 * 41
    return items


def test_every_start_residue_and_length():
    items = geometry_items(random.Random(3310))
    dev, doff = to_dev(*pack_items(items))
    assert dev.data_ptr() % 16 == 0
    for name in ("five", "twelve"):
        want = member_masks(SETS[name], dev, doff, 0)
        assert len(set(want.tolist())) > 4
        for what, m in builds(SETS[name]):
            same(run(m, dev, doff), want, (name, what), items)


def test_planted_geometry():
    """A match across a 16-byte boundary; a would-be match across two items; every bit found inside a wide load."""
    pats = ["ab+c", "k(1|10|100)"]
    z = b"z"
    items = [z * 14 + b"abbc" + z * 22,                  # starts at 0: the match lies in bytes 14 .. 17, across the boundary
             z * 3 + b"ab",                              # ... "ab" | "c": the two halves of a match in two items
             b"c" + z * 4 + b"k",
             b"1" + z * 2,                               # ("k" | "1" as well)
             z * 10,                                     # (54 .. 64: the next item starts on a boundary)
             b"zabck1" + z * 42,                         # both bits are in by byte 6 of a 16-byte load; the rest adds nothing
             b"abck100abck1" * 4,                        # ... and would set the same bits again
             z * 7 + b"k10" + z * 5 + b"abc"]            # first one bit, then across the next boundary the other
    assert sum(len(it) for it in items[:5]) == 64 and all(len(it) == 48 for it in items[5:7])
    want = np.array([1, 0, 0, 0, 0, 3, 3, 3], dtype=np.uint32)
    dev, doff = to_dev(*pack_items(items))
    same(member_masks(pats, dev, doff, 0), want, "members", items)
    for what, m in [("default", rr.RMulti(pats)), ("cut", rr.RMulti(pats, max_rows=4)), ("global", rr.RMulti(pats, engine=rr.ENGINE_DFA_GLOBAL))]:
        same(run(m, dev, doff), want, what, items)
    assert rr.RMulti(pats, max_rows=4).groups == 2
    # with a separator: "za" + [b] + "czz" - the separator would complete the match, and is never read
    dev, doff = to_dev(*pack_items([b"za", b"czz", b"zab"], trim=1, sep=b"b"))
    for what, m in [("default", rr.RMulti(pats)), ("global", rr.RMulti(pats, engine=rr.ENGINE_DFA_GLOBAL))]:
        same(run(m, dev, doff, trim=1), np.zeros(3, dtype=np.uint32), what)


def test_trims():
    pats, items = SETS["nullable"], items_of("nullable")[:300]
    dev, doff = to_dev(*pack_items(items, trim=1, sep=b"c"))
    m = rr.RMulti(pats)
    for trim in (0, 1, 2, 100):
        want = member_masks(pats, dev, doff, trim)
        same(run(m, dev, doff, trim=trim), want, trim)
    assert (want == 1).all()                            # trim beyond every item: only the nullable member's bit


def test_counts_and_planes():
    pats = SETS["thirtytwo"]
    m = rr.RMulti(pats)
    for n in (1, 65, 3001):
        base = items_of("thirtytwo")
        items = [base[(5 * i) % len(base)] for i in range(n)]
        dev, doff = to_dev(*pack_items(items))
        masks = m.contains_extents(dev, doff)
        host = masks.cpu().numpy().view(np.uint32)
        same(host, member_masks(pats, dev, doff, 0), n)
        counts = m.counts(masks).cpu().numpy()
        assert counts.tolist() == [int(((host >> np.uint32(k)) & 1).sum()) for k in range(32)], n
        nw = (n + 31) // 32
        for k in (0, 1, 11, 31):
            out = torch.full((nw + GUARD,), POISON, dtype=torch.int32, device="cuda")
            plane = m.plane(masks, k, out=out)
            assert torch.equal(plane, member(pats[k]).contains_extents_bits(dev, doff)), (n, k)         # word for word
            assert (out[nw:] == POISON).all()
            assert rr.bitmap_count(plane, n) == int(counts[k])
    assert len(m.counts(masks)) == 32 and len(rr.RMulti(pats[:5]).counts(masks)) == 5


def test_empty_languages_cost_a_memset_and_an_empty_batch_nothing():
    items = items_of("one")[:100]
    dev, doff = to_dev(*pack_items(items))
    same(run(rr.RMulti(["[]", "[]"]), dev, doff), np.zeros(100, dtype=np.uint32), "the empty languages")
    same(run(rr.RMulti(["[]", "ab+c"], max_rows=1), dev, doff), member_masks(["[]", "ab+c"], dev, doff, 0), "an empty first group")
    buf = guarded(0)
    rr.RMulti(["a"]).contains_extents(dev, doff[:1], out=buf)
    torch.cuda.synchronize()
    assert (buf == POISON).all()


def test_a_side_stream_and_a_captured_graph():
    pats, items = SETS["twelve"], items_of("twelve")
    dev, doff = to_dev(*pack_items(items, trim=1))
    m = rr.RMulti(pats, max_rows=8)
    assert m.groups >= 3
    want = want_masks("twelve")
    eager = m.contains_extents(dev, doff, trim=1).clone()
    same(eager.cpu().numpy().view(np.uint32), want, "eager")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    out = guarded(len(items))
    got = m.contains_extents(dev, doff, trim=1, out=out, stream=side)
    side.synchronize()
    assert torch.equal(got, eager) and (out[len(items):] == POISON).all()
    out.fill_(0)
    with torch.cuda.stream(side):
        m.contains_extents(dev, doff, trim=1, out=out)                     # (tables are up, nothing is allocated inside the capture)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            m.contains_extents(dev, doff, trim=1, out=out)
    torch.cuda.current_stream().wait_stream(side)
    out.fill_(POISON)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[:len(items)], eager) and (out[len(items):] == POISON).all()


def large_batch(pats, seed, nbytes=4 << 20):
    """About 4 MiB of items of 0 .. 120 bytes over the members' alphabet, a member's shortest match planted in one item in three."""
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"abcxk01.d@yz:/hftps \n\x00\xff", dtype=np.uint8)
    text = alphabet[rng.integers(0, len(alphabet), size=nbytes)]
    lens = rng.integers(0, 121, size=nbytes // 50)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    offs = offs[offs <= nbytes]
    needles = []
    for p in dict.fromkeys(pats):
        w = shortest_accepted(oracle_for(p))
        if w:
            needles.append(np.frombuffer(w.replace(b"x", b"\n") if "\n" in p else w, dtype=np.uint8))
    for i in range(0, len(offs) - 1, 3):
        nd = needles[(i // 3) % len(needles)]
        b, e = int(offs[i]), int(offs[i + 1])
        if e - b >= len(nd):
            at = b + int(rng.integers(0, e - b - len(nd) + 1))
            text[at:at + len(nd)] = nd
    return text[:int(offs[-1])].copy(), offs


@pytest.mark.parametrize("name", list(SETS))
def test_a_large_batch_against_the_members(name):
    pats = SETS[name]
    text, offs = large_batch(pats, 3320 + len(name))
    assert len(text) > 3 << 20 and len(offs) > 50_000
    dev, doff = to_dev(text, offs)
    want = member_masks(pats, dev, doff, 0)
    for k, p in enumerate(pats):                         # every member that can show both verdicts does
        col = int(((want >> np.uint32(k)) & 1).sum())
        assert (col == len(want)) if member(p).accepts_empty else (0 < col < len(want)), (name, k, col)
    same(run(rr.RMulti(pats), dev, doff), want, (name, "default"))
    same(run(rr.RMulti(pats, max_rows=16), dev, doff), want, (name, "cut"))
