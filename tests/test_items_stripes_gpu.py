"""The stripe-wise items kernels on the device (kernels_items.hip: item_index_kernel, match_items_stripes_kernel<1> and <2>,
match_items_stripes2_kernel) on the batches of tests/items_stripe_cases.py: marks on chosen bytes of a stripe, a round, a slot and a
pair, in the bitmap word two index workgroups share, across the index kernel's LDS tiles and past the result window - on every route
an indexed batch can take; stripes of 1024, 2048 and 4096 bytes on a block tiled on the device; and the one-call form on an upper
bound that is larger than the batch.  Every expectation is the oracle's (items_stripe_cases.expect)."""
import numpy as np
import pytest

import items_stripe_cases as isc
import roaringregex_amd as rr
from contains_cases import unpack

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

POISON_BYTE, POISON_WORD = 0xA5, -1


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"


_REGEX = {}


def regex(pattern, engine=rr.ENGINE_AUTO, stride2=True):
    key = (pattern, engine, stride2)
    if key not in _REGEX:
        r = rr.RRegex(pattern, engine)
        if not stride2:
            r.set_items_stride2(False)
        _REGEX[key] = r
    return _REGEX[key]


def match_routes(lang, trim):
    """-> [(name, regex)]: the kernels an indexed batch reaches through match_items"""
    auto = regex(lang.match)
    assert auto.engine == rr.ENGINE_DFA
    if trim == 0:
        return [("match, trim 0, byte stride <2>", auto)]
    assert auto.program(rr.PROGRAM_DFA2_ITEMS) is not None
    forced = regex(lang.match, rr.ENGINE_DFA)
    assert forced.engine == rr.ENGINE_DFA and forced.program(rr.PROGRAM_DFA2_ITEMS) is None
    return [("match, trim 1, stride 2", auto), ("match, trim 1, byte stride <1>, stride 2 switched off", regex(lang.match, stride2=False)),
            ("match, trim 1, byte stride <1>, ENGINE_DFA", forced)]


def contains_routes(lang, trim):
    auto = regex(lang.contains)
    if trim == 0:
        return [("contains, trim 0, byte stride <2>", auto)]
    assert auto.program(rr.PROGRAM_CONTAINS_DFA2_ITEMS) is not None
    return [("contains, trim 1, stride 2", auto), ("contains, trim 1, byte stride <1>, stride 2 switched off", regex(lang.contains, stride2=False))]


def first_bad(got, want):
    bad = np.nonzero(got != want)[0]
    return None if bad.size == 0 else (int(bad[0]), "of", int(bad.size), "got", int(got[bad[0]]))


def run_routes(batch):
    """The batch, indexed once, through every route of its trim; results into poisoned buffers longer than needed."""
    n = len(batch.offs) - 1
    nw = (n + 31) // 32
    dev, doff = torch.from_numpy(batch.text).cuda(), torch.from_numpy(batch.offs).cuda()
    items = rr.Items(dev, doff, trim=batch.trim)
    assert items.stripe_wise and items.num_items == n, batch.name
    want = isc.expect(batch, "match")
    for route, r in match_routes(batch.lang, batch.trim):
        out = torch.full((n + 80,), POISON_BYTE, dtype=torch.uint8, device="cuda")
        got = r.match_items(items, out=out)
        assert got.numel() == n
        assert first_bad(got.cpu().numpy(), want) is None, (batch.name, route, "first bad item", first_bad(got.cpu().numpy(), want))
        assert bool((out[n:] == POISON_BYTE).all()), (batch.name, route, "bytes behind the result were written")
    want = isc.expect(batch, "contains")
    for route, r in contains_routes(batch.lang, batch.trim):
        out = torch.full((nw + 9,), POISON_WORD, dtype=torch.int32, device="cuda")
        bits = r.contains_items_bits(items, out=out)
        assert bits.numel() == nw
        got = unpack(bits.cpu().numpy(), n)
        assert first_bad(got, want) is None, (batch.name, route, "first bad item", first_bad(got, want))
        if n & 31:
            assert (int(bits[-1].item()) & 0xffffffff) >> (n & 31) == 0, (batch.name, route, "bits beyond the last item")
        assert bool((out[nw:] == POISON_WORD).all()), (batch.name, route, "words behind the bitmap were written")
    # the lane-per-item route must agree too (not the reference: a second witness)
    lanes = regex(batch.lang.match).match_extents(dev, doff, trim=batch.trim).cpu().numpy()
    assert first_bad(lanes, isc.expect(batch, "match")) is None, (batch.name, "lane per item")


@pytest.mark.parametrize("trim", (0, 1))
@pytest.mark.parametrize("family", isc.SMALL_FAMILIES)
def test_small_families_on_every_route(family, trim):
    for batch in isc.small_cases(family, trim):
        run_routes(batch)


def test_the_window_case_passes_the_byte_stride_window_on_the_wide_tables_only():
    """What family D's two languages are for: an items table past 16 KiB leaves the byte-stride kernels a result window of fewer than
    16384 words, which a workgroup of one-byte items passes; a table of a few rows leaves one that it does not."""
    wide, small = isc.DENSE_WIDE, isc.DENSE_SMALL
    assert regex(wide.match).useful_states >= isc.WIDE_ROWS and regex(wide.contains).contains_states >= isc.WIDE_ROWS
    assert regex(small.match).useful_states <= 4 and regex(small.contains).contains_states <= 4
    row_bytes = 131 * 4                                               # device.hpp:236 kItemColumns entries of four bytes
    per_workgroup = isc.THREADS * isc.STRIPE // 32                    # result words of a workgroup of one-byte items
    assert (80 * 1024 - isc.WIDE_ROWS * row_bytes) // 4 < per_workgroup <= (80 * 1024 - 4 * row_bytes) // 4       # kernels_items.hip:466-467


# ------------------------------------------------------------------------------------------------------------ stripes other than 512
def tile_on_device(block, copies):
    """`copies` copies of the block, made on the device -> (text, offsets)"""
    nb, n = len(block.text), len(block.offs) - 1
    text = torch.from_numpy(block.text).cuda().repeat(copies)
    starts = torch.from_numpy(block.offs[:-1]).cuda()
    offs = (torch.arange(copies, dtype=torch.int64, device="cuda")[:, None] * nb + starts[None, :]).reshape(-1)
    offs = torch.cat([offs, torch.tensor([copies * nb], dtype=torch.int64, device="cuda")]).contiguous()
    assert offs.numel() == copies * n + 1
    return text, offs


def stripe_of(nbytes, offs):
    """The stripe stripe_for_lines gives `nbytes` bytes of as many items: that of a corpus of the same size with a '\\n' on every item's last byte."""
    buf = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    buf[offs[1:] - 1 - offs[0]] = 10
    corpus = rr.Corpus(buf)
    assert corpus.num_lines == offs.numel() - 1
    return corpus.stripe


def tiled_equals(got, want_block, copies):
    want = torch.from_numpy(want_block).cuda()
    return bool((got.view(copies, want.numel()) == want[None, :]).all())


def unpack_on_device(bits, n):
    shifts = torch.arange(32, dtype=torch.int32, device="cuda")
    return ((bits[:, None] >> shifts[None, :]) & 1).to(torch.uint8).reshape(-1)[:n]


@pytest.mark.parametrize("total,lengths,stripe", [(130 << 20, isc.SHORT_ITEMS, 1024), (260 << 20, isc.SHORT_ITEMS, 2048), (1 << 30, isc.LONG_ITEMS, 4096)])
def test_larger_stripes_on_a_tiled_block(total, lengths, stripe):
    """A block of 64 KiB and an odd byte, checked by the oracle, tiled on the device to 130 MiB, 260 MiB and 1 GiB: the stripe is 1024,
    2048 and 4096 bytes (asserted through a corpus of the same shape), and copy c lies c bytes further along it than copy 0."""
    for trim in (0, 1):
        block = isc.tiled_block(trim, lengths)
        nb, n = len(block.text), len(block.offs) - 1
        copies = -(-total // nb)
        assert copies >= 2 * stripe and isc.copies_meet_every_residue(nb, 2 * stripe, stripe)
        text, offs = tile_on_device(block, copies)
        assert text.numel() >= total
        assert stripe_of(text.numel(), offs) == stripe, (trim, "the stripe this batch was meant to have")
        items = rr.Items(text, offs, trim=trim)
        assert items.stripe_wise and items.num_items == copies * n
        got = regex(block.lang.match).match_items(items)
        assert tiled_equals(got, isc.expect(block, "match"), copies), (stripe, trim, "match", int(got.sum()))
        bits = regex(block.lang.contains).contains_items_bits(items)
        got = unpack_on_device(bits, copies * n)
        assert tiled_equals(got, isc.expect(block, "contains"), copies), (stripe, trim, "contains", int(got.sum()))
        del items, text, offs, got, bits
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------ the one-call form
def fresh_allocation(nbytes):
    """A tensor that is an allocation of its own: what is left of the allocation behind a byte of it is what is left of the tensor."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    t = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    seg = [s for s in torch.cuda.memory_snapshot() if s["address"] <= t.data_ptr() < s["address"] + s["total_size"]]
    assert len(seg) == 1 and seg[0]["address"] == t.data_ptr() and seg[0]["total_size"] == nbytes, "the tensor is not an allocation of its own"
    return t


def one_call(block, copies, pool, at, what):
    """The tiled block at byte `at` of `pool`, through match_extents and contains_extents_bits, against the tiled expectation."""
    text, offs = tile_on_device(block, copies)
    n = offs.numel() - 1
    pool[at:at + text.numel()] = text
    data = pool[at:]
    assert data.data_ptr() % 16 == 0
    out = torch.full((n + 80,), POISON_BYTE, dtype=torch.uint8, device="cuda")
    got = regex(block.lang.match).match_extents(data, offs, trim=block.trim, out=out)
    assert tiled_equals(got, isc.expect(block, "match"), copies), (what, "match", int(got.sum()))
    assert bool((out[n:] == POISON_BYTE).all()), (what, "bytes behind the result were written")
    nw = (n + 31) // 32
    out = torch.full((nw + 9,), POISON_WORD, dtype=torch.int32, device="cuda")
    bits = regex(block.lang.contains).contains_extents_bits(data, offs, trim=block.trim, out=out)
    assert tiled_equals(unpack_on_device(bits, n), isc.expect(block, "contains"), copies), (what, "contains")
    assert bool((out[nw:] == POISON_WORD).all()), (what, "words behind the bitmap were written")
    return text.numel(), offs


BOUND = 136 << 20


@pytest.mark.parametrize("where", ("front", "middle"))
def test_one_call_on_a_trusted_bound_with_another_stripe(where):
    """More than 1.1 M items of 8 bytes, 9 MiB, with 136 MiB of allocation from their first byte on: 128 bytes per item cover the bound,
    so index, stripe (1024, where the batch alone would have 512) and grid are laid out for it, and 127 MiB of stripes lie behind the
    batch's last byte."""
    for trim in (0, 1):
        block = isc.tiled_block(trim, isc.EIGHT_BYTE_ITEMS, nbytes=32 << 10)
        nb, n = len(block.text), len(block.offs) - 1
        copies = -(-BOUND // isc.PLAUSIBLE_PER_ITEM // n) + 1
        assert copies * n >= 1_100_000 and copies * n * isc.PLAUSIBLE_PER_ITEM >= BOUND and copies * n >= isc.STRIPES_MIN
        assert isc.STRIPES_MIN_BYTES <= copies * nb <= 12 << 20
        at = 0 if where == "front" else BOUND + 48
        pool = fresh_allocation(BOUND if where == "front" else 2 * BOUND)
        bound = pool.numel() - at
        assert BOUND - 48 <= bound <= min(BOUND, copies * n * isc.PLAUSIBLE_PER_ITEM)
        nbytes, offs = one_call(block, copies, pool, at, (where, trim))
        # the stripes: 1024 bytes for as many items in the bound, 512 for the batch's own extent
        ends = torch.linspace(1, bound, copies * n, dtype=torch.float64, device="cuda").to(torch.int64)
        assert stripe_of(bound, torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), ends])) == 1024
        assert stripe_of(nbytes, offs) == 512
        del pool, ends
    torch.cuda.empty_cache()


def test_one_call_unfit_on_the_device():
    """At least 65536 items, an allocation of 16 MiB - so the stripe-wise kernels are queued - and an extent below 8 MiB, which only the
    index pass sees: it raises the unfit flag, the stripe-wise kernel leaves its bitmap zero and the lane-per-item kernel answers."""
    for trim in (0, 1):
        block = isc.tiled_block(trim, isc.EIGHT_BYTE_ITEMS, nbytes=32 << 10)
        nb, n = len(block.text), len(block.offs) - 1
        copies = -(-70_000 // n)
        assert copies * n >= isc.STRIPES_MIN and copies * nb < isc.STRIPES_MIN_BYTES
        pool = fresh_allocation(16 << 20)
        assert pool.numel() >= isc.STRIPES_MIN_BYTES and pool.numel() <= max(copies * n * isc.PLAUSIBLE_PER_ITEM, 16 << 20)
        one_call(block, copies, pool, 0, ("unfit", trim))
        del pool
    torch.cuda.empty_cache()
