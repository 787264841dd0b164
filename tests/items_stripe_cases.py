"""Batches of explicit items for the stripe-wise items kernels (kernels_items.hip: item_index_kernel, match_items_stripes_kernel<1>,
<2>, match_items_stripes2_kernel) with an expectation that comes from the oracle alone.  Host only: numpy and the oracle.

A batch is one byte buffer and an offsets array; item i = text[offs[i] : offs[i + 1] - trim].  Its MARK is the byte the index kernel
sets a bit for: offs[i + 1] - 1, the item's last byte at trim 0 and its separator at trim 1.  Every builder below puts marks on
chosen bytes of a stripe, a round, a 16-byte slot, a pair, a bitmap word or an LDS tile of the index kernel, asserts that they are
there, and names them in Batch.features (feature -> the items whose mark is meant) so that tests/test_items_stripe_cases.py can move
the offset behind each by one byte and see the expectation change.

LANGUAGES.  FRAMED: match x[ab]*y, contains xa+y - x...y is accepted, x...a, a...y and a...a are not, so an end one byte early or
late turns two accepted neighbours into rejected ones.  DENSE_SMALL / DENSE_WIDE: for runs of one-byte and empty items, a? (an 'a' or
nothing) and c, alone and beside a 42-byte alternative that gives both tables 44 rows.  Match verdicts are OracleRegex.accepts on the
item, contains verdicts the brute force over its substrings (test_contains_items_lowering.contains_brute_force) up to 22 bytes and
Python's re beyond; items of at most one byte are looked up in a table of the same answers."""
import random
import re
from collections import namedtuple

import numpy as np

from pyoracle import OracleRegex
from test_contains_items_lowering import MAX_ITEM, contains_brute_force

STRIPE = 512                   # device.hpp:21 kMinStripe - what stripe_for_lines (device.hpp:37-44) gives below 128 MiB
ROUND = 128                    # device.hpp:45 kRound: bytes of a lane per round
SLOT = 16                      # kernels_items.hip:116 kSlots = kRound / 16: one uint4 of text, 16 mark bits, one flush test
PAIR, DWORD = 2, 4             # kernels_items.hip:255 (a step of the stride-2 kernel), :77 / :222 (a text word and its four marks)
THREADS = 1024                 # device.hpp:14-16 kThreads: stripes per workgroup of the items kernels
ENDS_ITEMS = 1024              # kernels_items.hip:314 kEndsItems: items per workgroup of item_index_kernel
ENDS_TILE = 4096               # kernels_items.hip:314 kEndsTile: bitmap words the index kernel assembles in LDS at a time
PICKUP = 32                    # kernels_items.hip:374 threadIdx.x < 32: the items in front of a workgroup's first that may share its first word
PAD_WORDS = 4                  # kernels_items.hip:365 (and :405) + 4: words behind the bitmap's last that the last workgroup writes
STRIPES_MIN = 65536            # items.cpp:13 kItemsStripesMin: items below which a one-call batch stays on a lane per item
STRIPES_MIN_BYTES = 8 << 20    # items.cpp:14 kItemsStripesMinBytes: bytes below which it does
PLAUSIBLE_PER_ITEM = 128       # items.cpp:54 items_extent_bound: the allocation's tail is trusted up to 128 bytes per item
TILE_BITS = ENDS_TILE * 32     # text bytes one LDS tile of the index kernel covers

SEPS = (b"x", b"y", b"a", b"\n", b";", b"\x00", b"\xff")      # trim 1: bytes the patterns take, and bytes they do not
ODD_BYTES = (0x00, 0x80, 0xc3, 0xff)


class Lang:
    """A match pattern and a contains pattern with the oracle's verdict per item, kept."""

    def __init__(self, match, contains, make):
        self.match, self.contains, self.make = match, contains, make
        self._o, self._memo, self._short = {}, {"match": {}, "contains": {}}, {}

    def oracle(self, kind):
        if kind not in self._o:
            self._o[kind] = OracleRegex(self.match if kind == "match" else self.contains)
        return self._o[kind]

    def verdict(self, kind, item):
        memo = self._memo[kind]
        if item not in memo:
            if kind == "match":
                memo[item] = int(self.oracle(kind).accepts(item))
            elif len(item) <= MAX_ITEM:
                memo[item] = contains_brute_force(self.oracle(kind), item)
            else:
                memo[item] = int(re.search(self.contains.encode(), item, re.S) is not None)
        return memo[item]

    def short_table(self, kind):
        """-> (verdict of the empty item, verdicts of the 256 one-byte items)"""
        if kind not in self._short:
            self._short[kind] = (self.verdict(kind, b""), np.array([self.verdict(kind, bytes([c])) for c in range(256)], dtype=np.uint8))
        return self._short[kind]


def _framed(n, accept, rng):
    """n bytes: accept 1 = x a...a y (both patterns take it), 2 = x [ab]... y (the match pattern alone), 0 = one of the rejected shapes"""
    if n <= 1:
        return (b"x", b"y", b"a")[rng.randrange(3)][:n]
    if accept and n == 2:
        return b"xy"
    if accept:
        return b"x" + (b"a" * (n - 2) if accept == 1 else (b"ab" * n)[:n - 2]) + b"y"
    return (b"x" + b"a" * (n - 1), b"a" * (n - 1) + b"y", b"a" * n)[rng.randrange(3)]


def _dense(n, accept, rng):
    if n <= 1:
        return b"aacb"[rng.randrange(4):][:1][:n]
    if accept and n == 42:
        return b"x" + (b"a" * 40 if accept == 1 else b"ab" * 20) + b"y"
    body = bytearray((b"ab" * n)[:n])
    if rng.randrange(3) == 0:
        body[rng.randrange(n)] = ord("c")
    return bytes(body)


FRAMED = Lang("x[ab]*y", "xa+y", _framed)
DENSE_SMALL = Lang("a?", "c", _dense)
DENSE_WIDE = Lang("a?|x[ab]{40}y", "c|xa{40}y", _dense)
WIDE_ROWS = 40                 # both tables of DENSE_WIDE have at least so many rows: past 16 KiB as a byte-stride items table

Batch = namedtuple("Batch", "name text offs trim lang features memo")


def marks(batch):
    """Positions of the items' marks, relative to the batch's first byte."""
    return batch.offs[1:] - 1 - batch.offs[0]


def item(batch, i, offs=None):
    offs = batch.offs if offs is None else offs
    return batch.text[offs[i]:offs[i + 1] - batch.trim].tobytes()


def expect(batch, kind):
    """The oracle's verdict per item, uint8."""
    if kind not in batch.memo:
        lens = np.diff(batch.offs) - batch.trim
        assert (lens >= 0).all()
        empty, one = batch.lang.short_table(kind)
        out = np.full(len(lens), empty, dtype=np.uint8)
        i1 = np.nonzero(lens == 1)[0]
        out[i1] = one[batch.text[batch.offs[i1]]]
        for i in np.nonzero(lens > 1)[0].tolist():
            out[i] = batch.lang.verdict(kind, item(batch, i))
        batch.memo[kind] = out
    return batch.memo[kind]


def moved(batch, k, d, kind):
    """The verdicts of items k and k + 1 with the offset between them moved by d, or None where that leaves an item without a byte for its mark."""
    offs = batch.offs.copy()
    offs[k + 1] += d
    if min(offs[k + 1] - offs[k], offs[k + 2] - offs[k + 1]) < max(batch.trim, 1):
        return None
    return tuple(batch.lang.verdict(kind, item(batch, i, offs)) for i in (k, k + 1))


def sensitive(batch, k, kind, every=False, both=True):
    """Items k and k + 1 are both accepted (both=False: item k is), the offset between them can move, and a legal move by one byte (every=True: each of them)
    changes the expectation."""
    want = expect(batch, kind)
    if k + 1 >= len(want) or not (want[k] and (want[k + 1] or not both)):
        return False
    got = [m != (want[k], want[k + 1]) for m in (moved(batch, k, +1, kind), moved(batch, k, -1, kind)) if m is not None]
    return bool(got) and (all(got) if every else any(got))


class Builder:
    def __init__(self, name, trim, lang=FRAMED, seed=1, filler=(4, 12)):
        self.name, self.trim, self.lang, self.rng, self.filler = name, trim, lang, random.Random(seed), filler
        self.chunks, self.ends, self.size, self.features = [], [], 0, {}

    @property
    def n(self):
        return len(self.ends)

    def make(self, n, accept=1):
        return self.lang.make(n, accept, self.rng)

    def add(self, body, sep=None, feature=None):
        """One item (its separator drawn from SEPS in turn); -> its number"""
        if self.trim:
            body = body + (SEPS[self.n % len(SEPS)] if sep is None else sep)
        assert body, "an item at trim 0 has a byte for its mark"
        self.chunks.append(body)
        self.size += len(body)
        self.ends.append(self.size)
        if feature:
            self.features.setdefault(feature, []).append(self.n - 1)
        return self.n - 1

    def add_total(self, total, accept=None):
        """An item that takes `total` bytes of the buffer, its separator included."""
        return self.add(self.make(total - self.trim, self.rng.randrange(3) if accept is None else accept))

    def add_run(self, totals, feature=None):
        """Items of one byte (total 1: empty at trim 1) and of two (trim 1 alone), all at once."""
        totals = np.asarray(totals, dtype=np.int64)
        assert totals.size and totals.min() >= 1 and totals.max() <= 1 + self.trim
        nbytes = int(totals.sum())
        data = np.frombuffer(b"aacb", dtype=np.uint8)[np.random.default_rng(self.rng.randrange(1 << 30)).integers(0, 4, size=nbytes)].copy()
        ends = np.cumsum(totals)
        if self.trim:
            data[ends - 1] = np.frombuffer(b"".join(SEPS), dtype=np.uint8)[(self.n + np.arange(len(totals))) % len(SEPS)]
        first = self.n
        self.chunks.append(data.tobytes())
        self.ends.extend((self.size + ends).tolist())
        self.size += nbytes
        if feature:                                      # (with the item in front: inside a run of one-byte items no offset can move)
            self.features.setdefault(feature, []).extend(range(max(first - 1, 0), self.n))
        return first

    def fill_to(self, size):
        """Filler items until the buffer holds `size` bytes."""
        lo, hi = self.filler
        assert size >= self.size, (self.name, size, self.size)
        while size - self.size > hi + lo:
            self.add_total(self.rng.randint(lo, hi))
        if size - self.size > hi:
            self.add_total((size - self.size) // 2)
        if size > self.size:
            self.add_total(size - self.size)
        assert self.size == size

    def fill_items_to(self, n):
        assert n >= self.n
        while self.n < n:
            self.add_total(self.rng.randint(*self.filler))

    def place(self, feature, body, residue, modulus, sep=None, front=5):
        """`body` with its mark at `residue` mod `modulus`, an accepted item of `front` bytes directly in front of it (asserted: a
        placement that is asked for is there)."""
        total, ftotal = len(body) + self.trim, front + self.trim
        start = self.size + ftotal + (residue - (self.size + ftotal + total - 1)) % modulus
        self.fill_to(start - ftotal)
        self.add(self.make(front, 1))
        k = self.add(body, sep, feature)
        assert (self.ends[k] - 1) % modulus == residue
        return k

    def place_at(self, feature, body, pos, front=5):
        """The same with the mark at the absolute position `pos`."""
        total, ftotal = len(body) + self.trim, front + self.trim
        self.fill_to(pos + 1 - total - ftotal)
        self.add(self.make(front, 1))
        k = self.add(body, sep=None, feature=feature)
        assert self.ends[k] - 1 == pos
        return k

    def finish(self, mod32=None):
        if mod32 is not None:
            while self.n % 32 != mod32:
                self.add_total(self.rng.randint(*self.filler))
        text = np.frombuffer(b"".join(self.chunks), dtype=np.uint8).copy()
        offs = np.concatenate([[0], self.ends]).astype(np.int64)
        assert len(text) == offs[-1] and (np.diff(offs) >= max(self.trim, 1)).all()
        return Batch(self.name, text, offs, self.trim, self.lang, self.features, {})


def both_accepted(batch):
    """Marks of the items that are accepted and followed by an accepted one, for match and for contains."""
    out = {}
    for kind in ("match", "contains"):
        w = expect(batch, kind)
        out[kind] = marks(batch)[:-1][(w[:-1] & w[1:]) == 1]
    return out


# ------------------------------------------------------------------------------------------------------------ A. every end position
def every_end_case(trim):
    """A mark on every byte of a stripe - so on every byte of a round, a slot, a text word and a pair - between two accepted items: six
    items of 41 bytes in all, 512 times (41 is coprime to 512: the first item's mark walks through all residues)."""
    b = Builder("A every end, trim %d" % trim, trim, seed=101)
    for _ in range(STRIPE):
        for total, accept in ((5, 1), (7, 1), (12, 1), (9, 0), (6, 1), (2, 0)):
            b.add_total(total, accept)
    batch = b.finish()
    assert len(batch.offs) - 1 == 6 * STRIPE and (len(batch.offs) - 1) % 32 == 0
    for kind, at in both_accepted(batch).items():
        assert len(set((at % STRIPE).tolist())) == STRIPE, (kind, "an end on every byte of a stripe, accepted items on both sides")
    batch.features["every_end"] = [int(k) for k in range(0, 6 * STRIPE, 6)]
    return batch


# ------------------------------------------------------------------------------------------------------------ B. straddling items
STRADDLE_SPANS = (1, 2, 40)
STRADDLE_BEHIND = tuple(range(41))


def straddle_case(trim):
    """Items that start in stripe g and have their mark d = 0 ... 40 bytes behind the first byte of stripe g + 1, g + 2 and g + 40 (the
    stripes between hold no end at all); marks on the last byte of a stripe; at trim 1 a body that ends on a stripe's last byte with its
    separator the next stripe's first byte, alone and with an empty item right behind it."""
    b = Builder("B straddling, trim %d" % trim, trim, seed=102)
    g = 1
    for span in STRADDLE_SPANS:
        for d in STRADDLE_BEHIND:
            b.fill_to(STRIPE * g + 300 + d % 7 - (5 + trim))
            b.add(b.make(5, 1))
            pos = STRIPE * (g + span) + d
            k = b.add(b.make(pos + 1 - trim - b.size, 1 if d % 3 != 2 else 0), feature="straddle_%d" % span)
            assert b.ends[k] - 1 == pos and (b.ends[k - 1]) // STRIPE == g
            b.add(b.make(5 + d % 3, 1))
            g = b.size // STRIPE + 2
    for j in range(3):
        b.place("stripe_last_byte", b.make(6 + j, 1), STRIPE - 1, STRIPE)
        b.add(b.make(4, 1))
        b.place("stripe_first_byte", b.make(6 + j, 1), 0, STRIPE, front=5 + j)
        b.add(b.make(4, 1))
        if trim:
            k = b.place("two_ends_in_a_pair", b.make(7 + j, 1), 0, STRIPE, front=3 + j)
            b.add(b"")
            b.add(b.make(4, 1))
            assert b.ends[k + 1] - 1 == b.ends[k]
    batch = b.finish(mod32=1)
    m = marks(batch)
    for span in STRADDLE_SPANS:
        ks = np.array(batch.features["straddle_%d" % span])
        assert sorted((m[ks] % STRIPE).tolist()) == list(STRADDLE_BEHIND)
        assert ((m[ks] // STRIPE - batch.offs[ks] // STRIPE) == span).all()
    return batch


# ------------------------------------------------------------------------------------------------------------ C. buffer ends
EXTENT_RESIDUES = tuple(range(1, 18)) + (127, 128, 129, 255, 511, 0)
PARTIAL_LAST_STRIPE = tuple(range(1, 18))
SHORT_EXTENTS = (1, 2, 3, 15, 16, 17, 37, 100, 511)
ONE_ITEM_EXTENTS = (1, 2, 5, 16, 17, 511, 512, 513, 700, 1025)


def buffer_end_cases(trim):
    """Small batches: an extent of each residue of EXTENT_RESIDUES mod 512, closed by short items and closed by an item that straddles
    into a last stripe of 1 ... 17 bytes; batches shorter than a stripe; batches of one item."""
    out = []
    for r in EXTENT_RESIDUES:
        b = Builder("C extent %d mod 512, trim %d" % (r, trim), trim, seed=300 + r)
        b.fill_to(2 * STRIPE + (r or STRIPE) - (5 + trim))
        b.add(b.make(5, 1), feature="extent")
        out.append(b.finish())
        assert len(out[-1].text) % STRIPE == r
    for r in PARTIAL_LAST_STRIPE:
        b = Builder("C last item into a stripe of %d, trim %d" % (r, trim), trim, seed=330 + r)
        b.fill_to(2 * STRIPE - 100)
        b.add(b.make(100 + r - trim, 1 if r % 2 else 0), feature="partial_last_stripe")
        out.append(b.finish())
        assert len(out[-1].text) == 2 * STRIPE + r and out[-1].offs[-2] < 2 * STRIPE
    for n in SHORT_EXTENTS:
        b = Builder("C batch of %d bytes, trim %d" % (n, trim), trim, seed=360 + n, filler=(1 + trim, 6))
        b.fill_to(max(n - (4 + trim), 0))
        b.add(b.make(n - b.size - trim, 1), feature="short_batch")
        out.append(b.finish())
        assert len(out[-1].text) == n < STRIPE
    for n in ONE_ITEM_EXTENTS:
        b = Builder("C one item of %d bytes, trim %d" % (n, trim), trim, seed=390 + n)
        b.add(b.make(n - trim, 1 if n % 3 else 0), feature="one_item")
        out.append(b.finish())
        assert len(out[-1].offs) == 2
    return out


# ------------------------------------------------------------------------------------------------------------ D. dense ends
SHORT_RUNS = (15, 16, 17)
LONG_RUN = 4096 + 64
WINDOW_TEXT = 3 * THREADS * STRIPE        # three workgroups of text


def _run_totals(n, trim, rng, packed=False):
    """n dense items: one byte each at trim 0; at trim 1 empty items and one-byte items mixed, 48 empty ones (16 marks in a slot
    whatever the alignment) then 16 of two bytes in all, then a random stretch (packed: 112 empty ones, 16 of two bytes)."""
    if not trim:
        return np.ones(n, dtype=np.int64)
    out = []
    while len(out) < n:
        out += [1] * 112 + [2] * 16 if packed else [1] * 48 + [2] * 16 + [rng.choice((1, 1, 2)) for _ in range(33)]
    return np.array(out[:n], dtype=np.int64)


def full_slots(batch):
    """Number of 16-byte slots in which every byte carries a mark."""
    m = marks(batch)
    per_slot = np.bincount(m // SLOT)
    return int((per_slot == SLOT).sum())


def dense_runs_case(trim, lang=DENSE_SMALL):
    """A run of 4160 dense items, and runs of 15, 16 and 17 one-byte steps (trim 1: empty items) that begin at every byte of a slot."""
    b = Builder("D dense runs, trim %d, %s" % (trim, lang.match), trim, lang, seed=104, filler=(20, 60))
    b.add(b.make(42, 1))
    b.add_run(_run_totals(LONG_RUN, trim, b.rng), feature="long_run")
    starts = {}
    for n in SHORT_RUNS:
        for a in range(SLOT):
            b.fill_to(b.size + 20 + (a - b.size - 20 - 42 - trim) % SLOT)
            b.add(b.make(42, 1))
            first = b.add_run([1] * n + [2] * trim, feature="run_%d" % n)      # (trim 1: closed by a one-byte item, an offset that can move)
            starts[(n, a)] = first
    b.add(b.make(42, 1))
    batch = b.finish(mod32=31)
    m = marks(batch)
    for (n, a), first in starts.items():
        assert m[first] % SLOT == a and (np.diff(m[first:first + n]) == 1).all()
    assert full_slots(batch) >= (2 * (LONG_RUN // 97) if trim else LONG_RUN // SLOT - 2), full_slots(batch)
    return batch


def window_case(trim, lang=DENSE_WIDE):
    """Three workgroups of text that is dense items only, behind a stretch of long items: 524288 results per workgroup at trim 0, more
    than any result window holds, the windows of the second and third workgroup far from word 0."""
    b = Builder("D window, trim %d, %s" % (trim, lang.match), trim, lang, seed=105, filler=(80, 120))
    for j in range(300):
        b.add(b.make(42, 1 + j % 2) if j % 3 else b.make(100, 0))
    front = b.n
    left = WINDOW_TEXT + 4096
    totals = _run_totals(left, trim, b.rng, packed=True)
    totals = totals[:int(np.searchsorted(np.cumsum(totals), left)) + 1]
    b.add_run(totals, feature="window_run")
    b.add(b.make(42, 1))
    batch = b.finish(mod32=1)
    assert batch.offs[-1] - batch.offs[front] >= WINDOW_TEXT and len(batch.text) <= 2 << 20
    per_group = np.bincount(marks(batch) // (THREADS * STRIPE))
    assert len(per_group) >= 4 and per_group[1:3].min() >= (THREADS * STRIPE) // 2, per_group
    return batch


# ------------------------------------------------------------------------------------------------------------ E. the shared word
FIRST_LENGTHS = tuple(range(1, 33))
EMPTY_BEFORE, EMPTY_BEHIND = 40, 4        # trim 1: so many items in front of item 1024 k are empty, and so many from it on
ITEM_COUNTS = (1023, 1024, 1025, 2049)


def _steps(b, upto):
    """One-byte steps up to item `upto`: trim 0 one-byte items; trim 1 empty items where the item number is at most EMPTY_BEFORE in front
    of a multiple of 1024 or less than EMPTY_BEHIND behind it, items of one byte (two with the separator) elsewhere."""
    j = np.arange(b.n, upto)
    totals = np.where(((j % ENDS_ITEMS) >= ENDS_ITEMS - EMPTY_BEFORE) | ((j % ENDS_ITEMS) < EMPTY_BEHIND), 1, 1 + b.trim)
    first = b.add_run(totals)
    for k in range(1, upto // ENDS_ITEMS + 1):
        if first <= ENDS_ITEMS * k - PICKUP and ENDS_ITEMS * k + EMPTY_BEHIND < upto:
            b.features.setdefault("pickup", []).extend(range(ENDS_ITEMS * k - PICKUP, ENDS_ITEMS * k + EMPTY_BEHIND))


def shared_word_cases(trim):
    """The bitmap word that holds the mark of item 1024 k - the first word the k-th index workgroup owns - also holds marks of the items
    in front of it: a first item of 1 ... 32 bytes shifts the word boundary through all 32 places among the 32 one-byte steps in front.
    (At most 31 of them share the word - with the mark of item 1024 k on its bit 31 -, never the 32nd: every item has a bit of its own.)"""
    out = []
    for r in FIRST_LENGTHS:
        b = Builder("E first item of %d bytes, trim %d" % (r, trim), trim, DENSE_WIDE, seed=500)
        b.add(b.make(r - trim, 0))
        _steps(b, 2 * ENDS_ITEMS + 60)
        out.append(b.finish())
    for k in (1, 2):
        seen = set()
        for batch in out:
            m = marks(batch)
            i = ENDS_ITEMS * k
            assert (np.diff(m[i - PICKUP:i + EMPTY_BEHIND]) == 1).all(), "32 one-byte steps in front of the workgroup's first item"
            seen.add(int(m[i]) % 32)
        assert len(seen) == 32, "the word boundary at each of the 32 places"
    for r in range(1, 33, 5):
        b = Builder("E 31 steps and a long item, first %d, trim %d" % (r, trim), trim, DENSE_WIDE, seed=510 + r, filler=(1 + trim, 9))
        b.add(b.make(r - trim, 0))
        b.fill_items_to(ENDS_ITEMS - 31)
        b.add_run(np.ones(31, dtype=np.int64), feature="steps_then_long")
        b.add(b.make(42, 1))
        assert b.n == ENDS_ITEMS + 1
        b.fill_items_to(ENDS_ITEMS + 50)
        out.append(b.finish())
        b = Builder("E a long item and 32 steps, first %d, trim %d" % (r, trim), trim, DENSE_WIDE, seed=520 + r, filler=(1 + trim, 9))
        b.add(b.make(r - trim, 0))
        b.fill_items_to(ENDS_ITEMS - 33)
        b.add(b.make(42, 1))
        b.add_run(np.ones(33, dtype=np.int64), feature="long_then_steps")
        assert b.n == ENDS_ITEMS + 1
        b.fill_items_to(ENDS_ITEMS + 50)
        out.append(b.finish())
    for n in ITEM_COUNTS:
        b = Builder("E %d items, trim %d" % (n, trim), trim, FRAMED, seed=530 + n)
        b.fill_items_to(n - 1)
        b.add(b.make(6, 1), feature="item_count")
        out.append(b.finish())
        assert len(out[-1].offs) - 1 == n
    return out


# ------------------------------------------------------------------------------------------------------------ F. LDS tiles
def index_ranges(batch):
    """What item_index_kernel's workgroups own: per workgroup (F, X) in bitmap words (kernels_items.hip:364-366, before the cap)."""
    m, n = marks(batch), len(batch.offs) - 1
    extent = int(batch.offs[-1] - batch.offs[0])
    out = []
    for i0 in range(0, n, ENDS_ITEMS):
        i1 = min(i0 + ENDS_ITEMS, n)
        out.append((0 if i0 == 0 else int(m[i0]) >> 5, int(m[i1]) >> 5 if i1 < n else ((extent + 31) >> 5) + PAD_WORDS))
    return out


def tile_case(trim):
    """Index workgroups whose 1024 items span several LDS tiles: marks on the last bit of a tile and the first of the next, an item of
    300 KiB that leaves a whole tile without a mark - in the first workgroup (tiles from bit 0), in a middle one (tiles from its own first
    word) and in the batch's last, whose range ends with the padding words."""
    b = Builder("F tiles, trim %d" % trim, trim, seed=106, filler=(280, 330))
    edges = []

    def edge(bit, both=True, first=False):
        """Marks on bit - 1 and on bit (an item of one byte, or an empty one and its separator); or on one of the two, between accepted items."""
        if both:
            k = b.place_at("tile_last_bit", b.make(40, 1), bit - 1)
            b.add(b"" if trim else b.make(1, 0), feature="tile_first_bit")
            edges.append((k, bit))
        else:
            b.place_at("tile_first_bit" if first else "tile_last_bit", b.make(40, 1), bit - (0 if first else 1))
        b.add(b.make(40, 1))

    edge(TILE_BITS)
    edge(TILE_BITS * 2, both=False)
    b.fill_items_to(ENDS_ITEMS)
    for last in (False, True):
        k0 = b.add_total(300)                                        # item 1024 / 2048: the workgroup's first
        assert k0 % ENDS_ITEMS == 0
        first_word = (b.ends[k0] - 1) >> 5
        b.add(b.make(5, 1))
        b.add(b.make(300 << 10, 1), feature="long_item")
        b.add(b.make(5, 1))
        for j in range(1 if last else 2):
            t = (b.size + 400 - first_word * 32) // TILE_BITS + 1
            edge(first_word * 32 + TILE_BITS * t, both=j == 0, first=True)
        b.fill_items_to(b.n + 20 if last else k0 + ENDS_ITEMS)
    batch = b.finish(mod32=31)
    m, ranges = marks(batch), index_ranges(batch)
    assert len(ranges) == 3 and all(x - f > ENDS_TILE for f, x in ranges), ranges
    assert ranges[-1][1] == ((len(batch.text) + 31) >> 5) + PAD_WORDS
    assert len(batch.text) <= 2 << 20
    words = m >> 5
    for k, bit in edges:
        f, x = ranges[k // ENDS_ITEMS]
        assert m[k] == bit - 1 and m[k + 1] == bit and (bit - f * 32) % TILE_BITS == 0 and f * 32 < bit < x * 32
    assert sorted(k // ENDS_ITEMS for k, _ in edges) == [0, 1, 2]
    assert len(batch.features["tile_last_bit"]) == 4 and len(batch.features["tile_first_bit"]) == 4
    for name, bit_of in (("tile_last_bit", TILE_BITS - 1), ("tile_first_bit", 0)):
        for k in batch.features[name]:
            assert (m[k] - ranges[k // ENDS_ITEMS][0] * 32) % TILE_BITS == bit_of, (name, k)
    for w, (f, x) in enumerate(ranges[1:], 1):                        # a whole tile without a mark
        tiles = [(t, min(t + ENDS_TILE, x)) for t in range(f, x, ENDS_TILE)]
        assert any(not ((words >= lo) & (words < hi)).any() for lo, hi in tiles if hi - lo == ENDS_TILE), w
    return batch


# ------------------------------------------------------------------------------------------------------------ G. rewritten bytes
def odd_bytes_case(trim):
    """0x00, 0x80, 0xc3 and 0xff at every byte of a slot: carrying a mark (an item's last byte at trim 0, its separator at trim 1), on
    either side of a marked byte, and inside an item."""
    b = Builder("G odd bytes, trim %d" % trim, trim, seed=107)
    for v in ODD_BYTES:
        x = bytes([v])
        for r in range(SLOT):
            b.place("odd_marked", b"xay" + x if not trim else b"xaay", r, SLOT, sep=x)
            b.add(b.make(4, 1))
            b.place("odd_in_front_of_mark", b"xaay" + x if trim else b"xay" + x + b"a", r, SLOT)
            b.add(b.make(4, 1))
            b.place("odd_behind_mark", b"xaay", r, SLOT)
            b.add(x + b"xay")
            b.place("odd_inside", b"xay" + x + b"xay", r, SLOT)
            b.add(b.make(5, 1))
    batch = b.finish(mod32=0)
    m, text = marks(batch), batch.text
    for name, shift in (("odd_marked", 0), ("odd_in_front_of_mark", -1), ("odd_behind_mark", 1), ("odd_inside", -(3 + trim))):
        at = m[np.array(batch.features[name])] + shift
        assert {(int(text[p]), int((p - shift) % SLOT)) for p in at} == {(v, r) for v in ODD_BYTES for r in range(SLOT)}, name
    return batch


SMALL_FAMILIES = ("A", "B", "C", "D", "E", "F", "G")


def small_cases(family, trim):
    """The batches of a family at one trim, in a list."""
    if family == "A":
        return [every_end_case(trim)]
    if family == "B":
        return [straddle_case(trim)]
    if family == "C":
        return buffer_end_cases(trim)
    if family == "D":
        return [dense_runs_case(trim, DENSE_SMALL), dense_runs_case(trim, DENSE_WIDE), window_case(trim, DENSE_WIDE), window_case(trim, DENSE_SMALL)]
    if family == "E":
        return shared_word_cases(trim)
    if family == "F":
        return [tile_case(trim)]
    if family == "G":
        return [odd_bytes_case(trim)]
    raise AssertionError(family)


# ------------------------------------------------------------------------------------------------------------ blocks to tile
BLOCK_BYTES = 64 << 10
SHORT_ITEMS = (1, 2, 3, 5, 8, 13, 21, 34, 55, 89)          # mean 23: at least 15 bytes per item (a 2048-byte stripe at 260 MiB)
LONG_ITEMS = (3, 40, 130, 200, 330, 600)                   # mean 217: above 128 bytes per item (a 4096-byte stripe at 1 GiB)
EIGHT_BYTE_ITEMS = (5, 8, 11, 7, 9, 8)                     # mean 8: the one-call batches


def tiled_block(trim, lengths, nbytes=BLOCK_BYTES, seed=108):
    """About `nbytes` of items whose sizes (separator included) are drawn from `lengths`, an odd number of bytes in all: copy c of the
    block starts c bytes further along the pairs, slots, rounds and stripes than copy 0.  A byte of ODD_BYTES in one item of eight."""
    b = Builder("block of %s, trim %d" % (lengths[:3], trim), trim, seed=seed)
    while b.size < nbytes:
        total = b.rng.choice(lengths)
        body = bytearray(b.make(max(total - trim, 1 - trim), b.rng.randrange(4) % 3))
        if body and b.n % 8 == 5:
            body[b.rng.randrange(len(body))] = b.rng.choice(ODD_BYTES)
        b.add(bytes(body))
    if b.size % 2 == 0:
        b.add(b.make(6 - trim, 1))
        if b.size % 2 == 0:
            b.add(b.make(5 - trim, 1))
    batch = b.finish()
    assert len(batch.text) % 2 == 1
    return batch


def copies_meet_every_residue(block_bytes, copies, stripe):
    """The starts of `copies` copies of a block of `block_bytes` bytes take every residue mod `stripe`."""
    return len({(c * block_bytes) % stripe for c in range(copies)}) == stripe
