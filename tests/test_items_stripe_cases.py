"""The batches of tests/items_stripe_cases.py on the CPU: every case puts its marks where its name says (by the mark's offset modulo the
pair, the text word, the slot, the round, the stripe, the bitmap word and the index kernel's LDS tile, or by the item's number modulo
1024), the expectation is the oracle's, it is neither all ones nor all zeros, and at every placement there is an offset between two
accepted items that changes the expectation when it moves by one byte."""
import re

import numpy as np
import pytest

import items_stripe_cases as isc
import roaringregex_amd as rr
from pyoracle import OracleRegex

# (family, feature, trim) without an offset that can move by a byte: a batch of one item; one-byte items alone at trim 0
NO_LEGAL_MOVE = {("C", "one_item", 0), ("C", "one_item", 1), ("E", "pickup", 0)}
# features whose mark is followed by an empty item at once: the item behind cannot be an accepted one
BEFORE_AN_EMPTY_ITEM = ("two_ends_in_a_pair",)
# families whose placements lie between items that BOTH patterns accept; elsewhere one of the two kinds must show the change
BOTH_KINDS = ("A", "B", "F")


def share_is_mixed(batches):
    for kind in ("match", "contains"):
        want = np.concatenate([isc.expect(b, kind) for b in batches])
        assert 0 < int(want.sum()) < len(want), (batches[0].name, kind, int(want.sum()), len(want))


def feature_is_sensitive(family, batches, name, trim):
    """Some instance of the feature, in some batch of the family, lies between two accepted items and moves the expectation."""
    found = {"match": False, "contains": False}

    def enough():
        return all(found.values()) if family in BOTH_KINDS else any(found.values())

    for b in batches:
        ks = b.features.get(name, ())
        for k in ks if len(ks) <= 600 else list(ks[:300]) + list(ks[::len(ks) // 300]):      # (a dense run: its first items and a sample)
            k = k - 1 if family == "C" or name == "item_count" else k        # (the feature is the batch's last item: the offset in front of it)
            for kind in found:
                if not found[kind] and k >= 0 and isc.sensitive(b, k, kind, every=family in ("A", "B"), both=name not in BEFORE_AN_EMPTY_ITEM):
                    found[kind] = True
            if enough():
                return
    assert enough(), (family, name, trim, found)


@pytest.mark.parametrize("trim", (0, 1))
@pytest.mark.parametrize("family", isc.SMALL_FAMILIES)
def test_small_families_place_their_marks_and_are_sensitive_to_them(family, trim):
    batches = isc.small_cases(family, trim)              # (the builders assert their own placements)
    share_is_mixed(batches)
    names = sorted({n for b in batches for n in b.features})
    assert names, family
    for name in names:
        if (family, name, trim) not in NO_LEGAL_MOVE:
            feature_is_sensitive(family, batches, name, trim)
    for b in batches:
        assert len(b.text) <= 2 << 20 and b.offs[0] == 0 and b.offs[-1] == len(b.text), b.name
        m = isc.marks(b)
        assert (np.diff(m) >= 1).all(), (b.name, "every item has a byte of its own for its mark")
        if trim:
            seps = set(b.text[m].tolist())
            assert len(b.offs) < 40 or seps >= {ord("x"), ord("y"), ord("a"), 10, ord(";"), 0, 0xff}, (b.name, seps)


def test_every_end_position_by_every_modulus():
    counts = set()
    for trim in (0, 1):
        counts |= {(len(b.offs) - 1) % 32 for b in (isc.every_end_case(trim), isc.straddle_case(trim), isc.dense_runs_case(trim))}
    assert counts >= {0, 1, 31}, "the results' last word full, with one bit and with 31 (expand_bits, copy_result_bits)"
    for trim in (0, 1):
        b = isc.every_end_case(trim)
        for kind, at in isc.both_accepted(b).items():
            for modulus in (isc.PAIR, isc.DWORD, isc.SLOT, isc.ROUND, isc.STRIPE, 32):
                assert len(set((at % modulus).tolist())) == modulus, (trim, kind, modulus)


def test_straddling_marks_by_stripe_slot_and_pair():
    for trim in (0, 1):
        b = isc.straddle_case(trim)
        m = isc.marks(b)
        for span in isc.STRADDLE_SPANS:
            ks = np.array(b.features["straddle_%d" % span])
            behind = m[ks] % isc.STRIPE
            assert set(behind.tolist()) == set(range(41))
            assert {int(x) // isc.SLOT for x in behind} == {0, 1, 2} and {int(x) % isc.PAIR for x in behind} == {0, 1}
            # no end at all in the stripes between the item's first and its last
            for k in ks[:3].tolist() if span == 1 else ks.tolist()[::7]:
                lo, hi = (b.offs[k] // isc.STRIPE + 1) * isc.STRIPE, m[k] // isc.STRIPE * isc.STRIPE
                assert not ((m >= lo) & (m < hi)).any() and (hi - lo) // isc.STRIPE == span - 1
        assert (m[np.array(b.features["stripe_last_byte"])] % isc.STRIPE == isc.STRIPE - 1).all()
        assert (m[np.array(b.features["stripe_first_byte"])] % isc.STRIPE == 0).all()
        if trim:
            ks = np.array(b.features["two_ends_in_a_pair"])
            assert (m[ks] % isc.STRIPE == 0).all() and (m[ks + 1] == m[ks] + 1).all() and (np.diff(b.offs)[ks + 1] == 1).all()


def test_buffer_ends():
    for trim in (0, 1):
        batches = isc.buffer_end_cases(trim)
        extents = [len(b.text) for b in batches if "extent" in b.features]
        assert sorted(e % isc.STRIPE for e in extents) == sorted(isc.EXTENT_RESIDUES) and min(extents) > 2 * isc.STRIPE
        assert {e % isc.PAIR for e in extents} == {0, 1} and {e % isc.SLOT for e in extents} == set(range(isc.SLOT))
        partial = [b for b in batches if "partial_last_stripe" in b.features]
        assert [len(b.text) - 2 * isc.STRIPE for b in partial] == list(isc.PARTIAL_LAST_STRIPE)
        assert all(b.offs[-2] // isc.STRIPE == 1 for b in partial), "the last item starts in the stripe in front of the partial one"
        assert [len(b.text) for b in batches if "short_batch" in b.features] == list(isc.SHORT_EXTENTS)
        assert [len(b.text) for b in batches if "one_item" in b.features] == list(isc.ONE_ITEM_EXTENTS)
        assert len(batches) == len(isc.EXTENT_RESIDUES) + len(isc.PARTIAL_LAST_STRIPE) + len(isc.SHORT_EXTENTS) + len(isc.ONE_ITEM_EXTENTS)


def test_dense_runs_and_windows():
    for trim in (0, 1):
        b = isc.dense_runs_case(trim)
        m = isc.marks(b)
        for n in isc.SHORT_RUNS:
            ks = np.array(b.features["run_%d" % n]).reshape(isc.SLOT, 1 + n + trim)[:, 1:]
            assert sorted((m[ks[:, 0]] % isc.SLOT).tolist()) == list(range(isc.SLOT)), "a run at every byte of a slot"
            assert (np.diff(m[ks[:, :n]], axis=1) == 1).all()
        assert isc.full_slots(b) >= 80
        w = isc.window_case(trim)
        per_workgroup = np.bincount(isc.marks(w) // (isc.THREADS * isc.STRIPE))
        # the stride-2 kernel's window is less than 46 KiB of LDS whatever the table: 376832 results
        assert per_workgroup[1] > 46 * 1024 * 8 and per_workgroup[2] > 46 * 1024 * 8, per_workgroup
        assert per_workgroup[0] > 10_000 and isc.marks(w)[300] > 10_000, "long items in front: the dense run starts off word 0"
    wide = isc.DENSE_WIDE
    assert rr.RRegex(wide.match).useful_states >= isc.WIDE_ROWS and rr.RRegex(wide.contains).contains_states >= isc.WIDE_ROWS
    assert rr.RRegex(isc.DENSE_SMALL.match).useful_states <= 4 and rr.RRegex(isc.DENSE_SMALL.contains).contains_states <= 4


def test_shared_word_by_item_number_and_bit():
    for trim in (0, 1):
        batches = isc.shared_word_cases(trim)
        first = [b for b in batches if b.name.startswith("E first item")]
        assert len(first) == 32
        for k in (1, 2):
            i = isc.ENDS_ITEMS * k
            assert {int(isc.marks(b)[i]) % 32 for b in first} == set(range(32))
            full = [b for b in first if isc.marks(b)[i] % 32 == 31]
            assert len(full) == 1 and (isc.marks(full[0])[i - 31:i + 1] >> 5 == isc.marks(full[0])[i] >> 5).all(), "31 marks from in front"
        for b in batches:
            for name in ("steps_then_long", "long_then_steps"):
                ks = b.features.get(name)
                if ks:
                    assert (ks[-1] + (1 if name == "steps_then_long" else 0)) % isc.ENDS_ITEMS == 0, (b.name, ks[-1])
        assert sorted(len(b.offs) - 1 for b in batches if "item_count" in b.features) == list(isc.ITEM_COUNTS)
        assert {(len(b.offs) - 1) % isc.ENDS_ITEMS for b in batches if "item_count" in b.features} >= {1023, 0, 1}


def test_tiles_of_the_index_kernel():
    for trim in (0, 1):
        b = isc.tile_case(trim)
        m, ranges = isc.marks(b), isc.index_ranges(b)
        assert [f for f, _ in ranges][0] == 0 and all(f % isc.ENDS_TILE for f, _ in ranges[1:]), "tiles from bit 0, and off it"
        for name, bit in (("tile_last_bit", isc.TILE_BITS - 1), ("tile_first_bit", 0)):
            ks = b.features[name]
            assert {k // isc.ENDS_ITEMS for k in ks} == {0, 1, 2}
            assert all((m[k] - ranges[k // isc.ENDS_ITEMS][0] * 32) % isc.TILE_BITS == bit for k in ks)
        assert all(np.diff(b.offs)[k] > 2 * isc.TILE_BITS for k in b.features["long_item"])
        assert (len(b.offs) - 1) // isc.ENDS_ITEMS == 2 and np.diff(b.offs).mean() > 128


def test_odd_bytes_at_every_byte_of_a_slot():
    for trim in (0, 1):
        b = isc.odd_bytes_case(trim)
        for v in isc.ODD_BYTES:
            at = np.nonzero(b.text == v)[0]
            assert len(set((at % isc.SLOT).tolist())) == isc.SLOT
            marked = np.intersect1d(at, isc.marks(b))
            assert len(set((marked % isc.SLOT).tolist())) == isc.SLOT, (trim, v, "carrying a mark")


def test_expectations_are_the_oracles():
    """expect() against OracleRegex.accepts and the brute force, item by item, without its tables of short items; Python's re (the
    expectation of items beyond 22 bytes) against the brute force on every item the brute force can take."""
    from test_contains_items_lowering import MAX_ITEM, contains_brute_force
    for trim in (0, 1):
        for b in (isc.every_end_case(trim), isc.odd_bytes_case(trim), isc.dense_runs_case(trim, isc.DENSE_WIDE), isc.shared_word_cases(trim)[30]):
            om, oc = OracleRegex(b.lang.match), OracleRegex(b.lang.contains)
            rc = re.compile(b.lang.contains.encode(), re.S)
            wm, wc = isc.expect(b, "match"), isc.expect(b, "contains")
            for i in range(0, len(wm), 1 if len(wm) < 4000 else 3):
                it = isc.item(b, i)
                assert wm[i] == int(om.accepts(it)), (b.name, i, it)
                if len(it) <= MAX_ITEM:
                    assert wc[i] == contains_brute_force(oc, it) == int(rc.search(it) is not None), (b.name, i, it)


def test_engines_the_gpu_routes_assert():
    for lang in (isc.FRAMED, isc.DENSE_SMALL, isc.DENSE_WIDE):
        r = rr.RRegex(lang.match)
        assert r.engine == rr.ENGINE_DFA and r.program(rr.PROGRAM_DFA2_ITEMS) is not None
        assert rr.RRegex(lang.contains).program(rr.PROGRAM_CONTAINS_DFA2_ITEMS) is not None
        forced = rr.RRegex(lang.match, rr.ENGINE_DFA)
        assert forced.program(rr.PROGRAM_DFA2_ITEMS) is None and rr.RRegex(lang.contains, rr.ENGINE_DFA).program(rr.PROGRAM_CONTAINS_DFA2_ITEMS) is None


@pytest.mark.parametrize("lengths,mean_at_least", [(isc.SHORT_ITEMS, 15), (isc.LONG_ITEMS, 129), (isc.EIGHT_BYTE_ITEMS, 7)])
def test_blocks_to_tile(lengths, mean_at_least):
    for trim in (0, 1):
        b = isc.tiled_block(trim, lengths)
        n, nbytes = len(b.offs) - 1, len(b.text)
        assert nbytes % 2 == 1 and isc.BLOCK_BYTES <= nbytes < isc.BLOCK_BYTES + 1024 and nbytes // n >= mean_at_least
        share_is_mixed([b])
        # as many copies as the smallest batch of each stripe has: every mark meets every byte of the stripe
        for stripe, total in ((1024, 130 << 20), (2048, 260 << 20), (4096, 1 << 30)):
            copies = -(-total // nbytes)
            assert copies >= 2 * stripe and isc.copies_meet_every_residue(nbytes, 2 * stripe, stripe)
        assert int((b.text >= 0x80).sum()) > 20 and int((b.text == 0).sum()) > 5
        m = isc.marks(b)
        both = isc.both_accepted(b)
        assert len(both["match"]) > 20 and len(both["contains"]) > 5
        ks = [int(k) for k in np.nonzero(np.isin(m, both["match"]))[0][:200]]
        assert any(isc.sensitive(b, k, "match") for k in ks)
