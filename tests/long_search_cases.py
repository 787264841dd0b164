"""Pattern families, closed-form references, the chunk-procedure model and the case sets for rrx_search_longest_string /
rrx_contains_string (one long string searched in chunks: kernels_long_search.hip, strings.cpp).  Shared by
test_search_longest_string_lowering.py (CPU) and test_search_longest_string_gpu.py (device).  Test infrastructure only.

  W(k)   = c((a|b){k})*d     a `c`, a run of a/b whose length is a multiple of k, a `d`.  The residue of the run rotates through
           k states in both tables, so the chunk maps never converge: the anchored table keeps k + 1 distinct prefix states (k = 5,
           7: every chunk flagged; k = 3: exactly the four slots), the starts table, which never dies, k + 2 (flagged for all three).
           A run one byte too long or too short is a DECOY: it looks like a match until the `d`.
  NUMBER = [0-9]+(\\.[0-9]+)?  a match of ANY length (every offset of a grid can be a start or an end), and an end that lies beyond
           a stretch in which the anchored table does not accept (after the '.').
  START_CASES' patterns (leftmost beats longer), a{1,300} (302 anchored states: the one-item path), a* and x?y?z? (nullable: no
  backward pass), k\\n+1 ('\\n' inside a match) and the URL pattern of patterns.py (large tables whose maps converge).

The texts are a filler that holds no byte of any pattern (z, q, blank, '\\n', and a NUL or a 0xC3 every few dozen bytes) with
matches and decoys PLANTED in it; the closed forms below (numpy) name the answer from the text alone, and the builders assert that
it is the match they planted.  The CPU file pins the closed forms to the sequential replay of the two program dumps and, at small
sizes, to the brute force.

The MODEL restates the chunked procedure from a DfaReplay of each table - chunk maps in walking order, the levels of groups of
128, the down-sweep to the entry state of every chunk, the extreme accepting offset per chunk, its reduction, and the forward
windows of strings.cpp - and can be run with ONE named defect."""
import functools

import numpy as np

import long_string_cases as L

SEARCH_FROM = 2048           # strings.cpp kLongSearchStringBytes: shorter strings are one item of the lane-per-item kernel
FIRST_WINDOW = 256           # strings.cpp kLongSearchFirstWindow
WINDOW_GROWTH = 15           # strings.cpp kLongSearchWindowGrowth
GROUP = L.K_LONG_GROUP
MAX_STATES = L.K_LONG_MAX_STATES
NONE = (-1, -1)

NUMBER = "[0-9]+(\\.[0-9]+)?"
A300, ASTAR, XYZ, KNL1 = "a{1,300}", "a*", "x?y?z?", "k\n+1"
LITERALS = {"abcd|c": (b"abcd", b"c"), "k100|0": (b"k100", b"0")}
ABC_B, NUM_DOT = "ab+c|b", "[0-9]+\\.[0-9]+|\\."


def W(k):
    return "c((a|b){%d})*d" % k


def url_pattern():
    import patterns
    return patterns.U2


# ------------------------------------------------------------------------------------------------ closed forms
def _arr(s):
    return np.frombuffer(s, dtype=np.uint8) if isinstance(s, (bytes, bytearray)) else np.asarray(s, dtype=np.uint8)


def _run_ends(mask, at):
    """For every index of `at` the end of the run of True in `mask` that begins there (the index itself where mask is False)."""
    stops = np.flatnonzero(~mask)
    at = np.atleast_1d(np.asarray(at, dtype=np.int64))
    j = np.searchsorted(stops, at)
    return np.where(j < stops.size, stops[np.minimum(j, max(stops.size - 1, 0))] if stops.size else mask.size, mask.size)


def closed_w(k, s):
    """The first `c` whose a/b run has a multiple of k bytes and ends in a `d`; from a `c` there is one candidate only."""
    s = _arr(s)
    cs = np.flatnonzero(s == ord("c"))
    if cs.size == 0:
        return NONE
    e = _run_ends((s == ord("a")) | (s == ord("b")), cs + 1)
    ok = (e < s.size) & ((e - cs - 1) % k == 0)
    ok[ok] = s[e[ok]] == ord("d")
    hit = np.flatnonzero(ok)
    return (int(cs[hit[0]]), int(e[hit[0]]) + 1) if hit.size else NONE


def _is_digit(s):
    return (s >= ord("0")) & (s <= ord("9"))


def closed_number(s):
    s = _arr(s)
    dig = _is_digit(s)
    first = np.flatnonzero(dig)
    if first.size == 0:
        return NONE
    b = int(first[0])
    e = int(_run_ends(dig, b)[0])
    if e + 1 < s.size and s[e] == ord(".") and dig[e + 1]:
        e = int(_run_ends(dig, e + 1)[0])
    return b, e


def closed_a300(s):
    s = _arr(s)
    first = np.flatnonzero(s == ord("a"))
    if first.size == 0:
        return NONE
    b = int(first[0])
    return b, min(int(_run_ends(s == ord("a"), b)[0]), b + 300)


def closed_astar(s):
    s = _arr(s)
    return 0, int(_run_ends(s == ord("a"), 0)[0]) if s.size else 0


def closed_xyz(s):
    s, e = _arr(s), 0
    for ch in b"xyz":
        if e < s.size and s[e] == ch:
            e += 1
    return 0, e


def closed_literals(lits, s):
    """An alternation of literals: the smallest start of any of them, then the longest literal that stands there."""
    t = _arr(s).tobytes()
    found = [t.find(x) for x in lits]
    if max(found) < 0:
        return NONE
    b = min(f for f in found if f >= 0)
    return b, b + max(len(x) for x in lits if t.startswith(x, b))


def closed_abc_b(s):
    """ab+c|b: the first `b`; the `a` in front of it starts the match if its b-run ends in a `c`."""
    s = _arr(s)
    first = np.flatnonzero(s == ord("b"))
    if first.size == 0:
        return NONE
    i = int(first[0])
    e = int(_run_ends(s == ord("b"), i)[0])
    if i > 0 and s[i - 1] == ord("a") and e < s.size and s[e] == ord("c"):
        return i - 1, e + 1
    return i, i + 1


def closed_num_dot(s):
    """[0-9]+\\.[0-9]+|\\.: the first '.'; the digit run in front of it starts the match if a digit follows the '.'."""
    s = _arr(s)
    first = np.flatnonzero(s == ord("."))
    if first.size == 0:
        return NONE
    j, dig = int(first[0]), _is_digit(s)
    if j > 0 and dig[j - 1] and j + 1 < s.size and dig[j + 1]:
        b = j - 1 - int(_run_ends(dig[:j][::-1], 0)[0]) + 1
        return b, int(_run_ends(dig, j + 1)[0])
    return j, j + 1


def closed_knl1(s):
    """k\\n+1: the first `k` whose run of '\\n' is not empty and ends in a `1`."""
    s = _arr(s)
    ks = np.flatnonzero(s == ord("k"))
    if ks.size == 0:
        return NONE
    e = _run_ends(s == 10, ks + 1)
    ok = (e < s.size) & (e > ks + 1)
    ok[ok] = s[e[ok]] == ord("1")
    hit = np.flatnonzero(ok)
    return (int(ks[hit[0]]), int(e[hit[0]]) + 1) if hit.size else NONE


def closed_form(pattern):
    """pattern -> the function that names its leftmost-longest match in a text (None: by construction only)."""
    for k in (3, 5, 7):
        if pattern == W(k):
            return lambda s, k=k: closed_w(k, s)
    if pattern in LITERALS:
        return lambda s, lits=LITERALS[pattern]: closed_literals(lits, s)
    return {NUMBER: closed_number, A300: closed_a300, ASTAR: closed_astar, XYZ: closed_xyz, ABC_B: closed_abc_b, NUM_DOT: closed_num_dot,
            KNL1: closed_knl1}.get(pattern)


# ------------------------------------------------------------------------------------------------ geometry, as the source lays it
long_chunk = L.long_chunk


def back_grid(n):
    """The chunk of the backward pass over n bytes and its boundaries, counted from the string's END: n - c * chunk."""
    chunk = long_chunk(n)
    return chunk, [n - c * chunk for c in range(1, (n + chunk - 1) // chunk)]


def forward_windows(start, n, skew=0):
    """[(first byte, length)] of the forward windows from `start` in a string of n bytes at an address = skew mod 16."""
    out, pos = [], start
    while pos < n:
        walked = pos - start
        ln = walked * WINDOW_GROWTH if walked else FIRST_WINDOW - ((skew + pos) & 15)
        ln = min(ln, n - pos)
        out.append((pos, ln))
        pos += ln
    return out


# ------------------------------------------------------------------------------------------------ the model
class Table:
    """A plain table of a program dump as the chunk kernels widen it: one column per byte value below 128, one for the rest."""

    def __init__(self, d):
        self.D, self.start = d.nstates, d.start
        self.next, self.acc = np.asarray(d.next, dtype=np.int64), np.asarray(d.acc, dtype=np.int64)
        self.col = np.asarray(d.cls, dtype=np.int32)[np.minimum(np.arange(256), 128)]
        assert self.D <= MAX_STATES


DEFECTS = ("entries_all_start", "downsweep_off_by_one", "wrong_extreme", "drop_first_byte_event", "drop_last_byte_event", "window_restart",
           "level2_next_group")


def _split(col, chunk):
    full = col.size // chunk
    return col[:full * chunk].reshape(full, chunk), col[full * chunk:]


def directional_run(t, data, backward, entered, row0_dead=False, defect=None):
    """long_run_dfa on the bytes `data`: (extreme, exit state); extreme as device.hpp states it (forwards the offset behind the
    byte, backwards the byte's own offset; None where the table never accepts)."""
    a = _arr(data)
    n = a.size
    assert n > 0
    w = t.col[a[::-1] if backward else a]                     # the columns in WALKING order
    chunk = long_chunk(n)
    nch = (n + chunk - 1) // chunk
    body, tail = _split(w, chunk)
    entry = np.full(nch, entered, dtype=np.int64)
    if nch > 1:
        # 1  chunk maps in walking order (the four-step build yields the same maps as stepping from every state)
        maps = np.tile(np.arange(t.D, dtype=np.int64), (nch, 1))
        for j in range(chunk):
            maps[:len(body)] = t.next[maps[:len(body)], body[:, j][:, None]]
        for c in tail:
            maps[len(body)] = t.next[maps[len(body)], c]
        # 2  up-sweep, every level kept, until a level has at most GROUP maps
        levels = [maps]
        while len(levels[-1]) > GROUP:
            cur = levels[-1]
            m = (len(cur) + GROUP - 1) // GROUP
            out = np.empty((m, t.D), dtype=np.int64)
            for g in range(m):
                src = g + 1 if (defect == "level2_next_group" and len(levels) == 2 and g + 1 < m) else g
                s = np.arange(t.D, dtype=np.int64)
                for k in range(src * GROUP, min((src + 1) * GROUP, len(cur))):
                    s = cur[k][s]
                out[g] = s
            levels.append(out)
        # 3  down-sweep: the top level is one group entered in the start state
        parent = np.array([entered], dtype=np.int64)
        for cur in reversed(levels):
            ent = np.empty(len(cur), dtype=np.int64)
            for g in range(len(parent)):
                s = parent[g]
                for k in range(g * GROUP, min((g + 1) * GROUP, len(cur))):
                    ent[k] = s
                    s = cur[k][s]
            parent = ent
        entry = parent
        if defect == "entries_all_start":
            entry = np.full(nch, entered, dtype=np.int64)
        elif defect == "downsweep_off_by_one":
            entry = np.concatenate([[entered], entry[:-1]])
    # 4  the last accepting event of every chunk in walking order (index of the byte inside the chunk), and its exit state
    st = entry.copy()
    last = np.full(nch, -1, dtype=np.int64)
    sizes = np.full(nch, chunk, dtype=np.int64)
    sizes[-1] = n - (nch - 1) * chunk
    for j in range(chunk):
        rows = len(body) if j >= tail.size else nch
        cols = body[:, j] if rows == len(body) else np.concatenate([body[:, j], tail[j:j + 1]])
        st[:rows] = t.next[st[:rows], cols]
        ev = t.acc[st[:rows]] != 0
        if defect == "drop_first_byte_event" and j == 0:
            ev[:] = False
        if defect == "drop_last_byte_event":
            ev &= sizes[:rows] - 1 != j
        last[:rows][ev] = j
    assert not row0_dead or (t.acc[0] == 0 and not t.next[0].any())
    # the reduction: the chunk walked LAST that has an event holds the extreme
    has = np.flatnonzero(last >= 0)
    if has.size == 0:
        return None, int(st[-1])
    k = int(has[0] if defect == "wrong_extreme" else has[-1])
    walked = k * chunk + int(last[k]) + 1                    # bytes walked up to and including the event's byte
    return (n - walked if backward else walked), int(st[-1])


def search_model(starts, anchored, nullable, data, skew=0, defect=None):
    """rrx_search_longest_string's chunk route on `data` (>= SEARCH_FROM bytes): (start, end) or NONE."""
    a = _arr(data)
    assert a.size >= SEARCH_FROM
    start = 0
    if not nullable:
        start, _ = directional_run(starts, a, True, starts.start, False, defect)
        if start is None:
            return NONE
    end, state = start, anchored.start
    for pos, ln in forward_windows(start, a.size, skew):
        if defect == "window_restart":
            state = anchored.start
        ext, state = directional_run(anchored, a[pos:pos + ln], False, state, True, defect)
        if ext is not None:
            end = pos + ext
        if state == 0:
            break
    return start, end


def contains_model(starts, nullable, data, defect=None):
    return True if nullable else directional_run(starts, _arr(data), True, starts.start, False, defect)[0] is not None


# ------------------------------------------------------------------------------------------------ texts
FILL = np.frombuffer(b"zq \n", dtype=np.uint8)


def filler(seed, n, alphabet=FILL):
    """n bytes that belong to no pattern here: z, q, blank, '\\n', and a NUL or a 0xC3 about every 61 bytes."""
    rng = np.random.default_rng(seed)
    t = alphabet[rng.integers(0, alphabet.size, size=n)].copy()
    odd = np.flatnonzero(rng.integers(0, 61, size=n) == 0)
    t[odd] = np.where(rng.integers(0, 2, size=odd.size) == 0, 0x00, 0xC3)
    return t


def w_run(k, nab, seed):
    """c, nab bytes of a/b, d: a match of W(k) exactly when nab is a multiple of k."""
    return np.concatenate([[ord("c")], L.ab(seed, nab), [ord("d")]]).astype(np.uint8)


def digits(seed, n):
    return (ord("0") + np.random.default_rng(seed).integers(0, 10, size=n)).astype(np.uint8)


def plant(t, at, piece):
    piece = _arr(piece)
    assert 0 <= at and at + piece.size <= t.size, (at, piece.size, t.size)
    t[at:at + piece.size] = piece


class Case:
    """One string: `pattern` on `data` has the leftmost-longest match `want` ((-1, -1): none).  skew: the string sits at an
    address = skew mod 16 on the device."""

    def __init__(self, tag, pattern, data, want=None, skew=0):
        self.tag, self.pattern, self.skew = tag, pattern, skew
        self.data = np.ascontiguousarray(data, dtype=np.uint8)
        fn = closed_form(pattern)
        got = fn(self.data) if fn else want
        assert want is None or tuple(want) == tuple(got), (tag, "planted", want, "closed form", got)
        self.want = tuple(int(x) for x in got)

    def __repr__(self):
        return "%s[%d bytes, want %s]" % (self.tag, self.data.size, self.want)


def fits_w(k, length):
    return length >= 2 and (length - 2) % k == 0


def w_text(k, n, start, length, seed, decoys=True, second=True):
    """Filler of n bytes with a W(k) match of `length` bytes at `start`; in front of it (where there is room) a decoy whose run is one
    byte too long, behind it a decoy one byte too short and a second true match."""
    assert fits_w(k, length)
    t = filler(seed, n)
    plant(t, start, w_run(k, length - 2, seed + 1))
    if decoys and start >= 3 * k + 4:
        plant(t, start - (3 * k + 3) - 1, w_run(k, 3 * k + 1, seed + 2))
    at = start + length + 1
    if decoys and at + 2 * k + 1 <= n:
        plant(t, at, w_run(k, 2 * k - 1, seed + 3))
        at += 2 * k + 2
    if second and at + k + 2 <= n:
        plant(t, at, w_run(k, k, seed + 4))
    return t


def number_text(n, start, length, seed, dot_at=None):
    """Filler with a digit run [start, start + length) (a '.' at offset dot_at of it) and a longer number further right."""
    t = filler(seed, n)
    d = digits(seed + 1, length)
    if dot_at is not None:
        assert 0 < dot_at < length - 1
        d[dot_at] = ord(".")
    plant(t, start, d)
    after = start + length + 2
    if after + 9 <= n:
        plant(t, after, b"1234.5678")
    return t


# ------------------------------------------------------------------------------------------------ case sets
POSITION_N = 256 * 300 + 40          # backwards 301 chunks of 256 bytes in 3 groups; forwards from a start near 0 the windows are
                                     # 256, 3840 (15 chunks) and 61440 bytes (240 chunks: two groups)
SPANS = {"one chunk": 100, "two chunks": 300, "130 chunks": 130 * 256 + 77}


def _near(p, lo, hi):
    return [q for q in (p - 1, p, p + 1) if lo <= q <= hi]


def start_positions(n, length):
    """Offsets for a match START: 0, the last that still fits, and the three around a chunk boundary (the nearest to the end, one in
    the middle) and around a group boundary of the BACKWARD grid."""
    chunk, bounds = back_grid(n)
    hi = n - length
    out = {0, hi}
    picks = [bounds[0], bounds[len(bounds) // 2]] + ([n - GROUP * chunk] if len(bounds) >= GROUP else [])
    for b in picks:
        out.update(_near(b, 0, hi))
    return sorted(out)


def end_offsets(start, n, skew=0):
    """Distances start -> END at the edges of the FORWARD grid: around every window hand-over, around the first chunk boundary inside
    every window of two chunks and more, and around its first group boundary."""
    out = set()
    for pos, ln in forward_windows(start, n, skew):
        out.update(_near(pos + ln, start + 1, n))
        chunk = long_chunk(ln)
        if ln > chunk:
            out.update(_near(pos + chunk, start + 1, n))
        if ln > GROUP * chunk:
            out.update(_near(pos + GROUP * chunk, start + 1, n))
    return sorted(e - start for e in out)


def number_position_cases():
    n, out = POSITION_N, []
    for name, length in SPANS.items():
        for s in start_positions(n, length):
            out.append(Case("number start at %d, %s" % (s, name), NUMBER, number_text(n, s, length, 11 + s % 89), (s, s + length)))
    for s in (0, 5, 256 * 40 + 3):
        for d in end_offsets(s, n):
            dot = d // 2 if d >= 3 else None
            out.append(Case("number from %d end at +%d" % (s, d), NUMBER, number_text(n, s, d, 17 + d % 97, dot), (s, s + d)))
    # the '.' as last byte of a chunk of the forward grid and as its first: the stretch without an accepting state crosses the edge
    for dot in (255, 256, 256 + 3840 - 1, 256 + 3840):
        out.append(Case("number '.' at +%d" % dot, NUMBER, number_text(n, 0, dot + 40, 23, dot), (0, dot + 40)))
    out.append(Case("number: a decoy `12.` only", NUMBER, _with(filler(29, n), 5000, b"12.z"), (5000, 5002)))
    out.append(Case("number: none", NUMBER, filler(31, n), NONE))
    return out


def _with(t, at, piece):
    plant(t, at, piece)
    return t


def w_position_cases(k):
    """W(k), every chunk flagged: the starts that the backward grid names, at the three spans, and the ends of the forward grid that
    a run of a multiple of k can reach."""
    n, out = POSITION_N, []
    for name, length in SPANS.items():
        length += (2 - length) % k
        for s in start_positions(n, length):
            out.append(Case("W(%d) start at %d, %s" % (k, s, name), W(k), w_text(k, n, s, length, 37 + s % 83), (s, s + length)))
    for s in (0, 1, 2, 3, 4, 5, 6):                          # the residue of start -> edge changes with the start: every edge is met
        for d in end_offsets(s, n):
            if fits_w(k, d):
                out.append(Case("W(%d) from %d end at +%d" % (k, s, d), W(k), w_text(k, n, s, d, 41 + d % 79), (s, s + d)))
    t = filler(43, n)
    plant(t, 300, w_run(k, 40 * k + 1, 44))                   # decoys alone: no match
    plant(t, n - 40 * k - 1, w_run(k, 40 * k - 1, 45))
    out.append(Case("W(%d) decoys only" % k, W(k), t, NONE))
    return out


GEOMETRY_LENGTHS = tuple(sorted(set(L.GEOMETRY_LENGTHS + (SEARCH_FROM - 1, SEARCH_FROM, SEARCH_FROM + 1))))


def geometry_cases():
    """Every length at which the chunking changes, and the hand-over threshold - 1, at it and + 1: W(5) with the match's start in the
    chunk walked last by the backward pass and its end in the last chunk of the string; a number that is the whole string; none."""
    out = []
    for n in GEOMETRY_LENGTHS:
        length = n - 7 - (n - 7 - 2) % 5
        out.append(Case("geometry W(5) n=%d" % n, W(5), w_text(5, n, 3, length, n % 71, decoys=False), (3, 3 + length)))
        out.append(Case("geometry number n=%d" % n, NUMBER, digits(n % 73, n), (0, n)))
        out.append(Case("geometry W(5) n=%d none" % n, W(5), _with(filler(n % 67, n), 1, w_run(5, 5 * ((n - 8) // 5) + 1, 3)), NONE))
    return out


def slot_cases():
    """W(3): 6 states, exactly the four slots.  W(5), W(7) at two-level lengths with decoys on both sides."""
    out = []
    for k in (3, 5, 7):
        for n in L.TWO_LEVEL_LENGTHS:
            length = 2 + k * ((n // 2) // k)
            s = n // 4 + 1
            out.append(Case("rotation W(%d) n=%d" % (k, n), W(k), w_text(k, n, s, length, k * 100 + n % 61), (s, s + length)))
        n = L.TWO_LEVEL_LENGTHS[0]
        out.append(Case("rotation W(%d) none" % k, W(k), _with(filler(k, n), 9, w_run(k, k * ((n - 20) // k) - 1, k)), NONE))
    return out


def start_cases():
    """Leftmost beats longer: START_CASES' items planted behind a filler, in the last chunk walked and across a chunk edge."""
    from test_search_longest_items_lowering import START_CASES
    wants = [(0, 4), (2, 6), (0, 4), (0, 4), (1, 5)]
    out, n = [], 256 * 9 + 13
    for (p, item), (ws, we) in zip(START_CASES, wants):
        for at in (0, 256 * 4 - 2, n - len(item)):
            t = filler(len(item) + at % 53, n)
            plant(t, at, item)
            out.append(Case("start case %s at %d" % (p, at), p, t, (at + ws, at + we)))
    t = filler(59, n)
    plant(t, 700, b"k\n\n\n1")
    plant(t, 300, b"k\nz1")
    out.append(Case("newline inside a match", KNL1, t, (700, 705)))
    out.append(Case("abcd|c none", "abcd|c", filler(61, n), NONE))
    return out


def handover_cases():
    """a{1,300}: 302 anchored states - the one-item path at every length, still exact (the cap at 300 included)."""
    out = []
    for n, s, run in ((SEARCH_FROM + 7, 100, 299), (256 * 200 + 77, 256 * 100 - 3, 300), (256 * 200 + 77, 256 * 100 - 3, 400), (256 * 9, 0, 256 * 9)):
        t = filler(67 + run, n)
        plant(t, s, np.full(run, ord("a"), dtype=np.uint8))
        out.append(Case("a{1,300} n=%d run=%d" % (n, run), A300, t, (s, s + min(run, 300))))
    out.append(Case("a{1,300} none", A300, filler(71, 256 * 9), NONE))
    return out


def nullable_cases():
    out, n = [], 256 * 140 + 9
    for run in (0, 1, 255, 256, 257, 256 + 3840, n):
        t = filler(73, n)
        plant(t, 0, np.full(run, ord("a"), dtype=np.uint8))
        if run + 2 < n:
            plant(t, run + 1, b"aaaa"[:n - run - 1])
        out.append(Case("a* run=%d" % run, ASTAR, t, (0, run)))
    for head, e in ((b"xyz", 3), (b"xz", 2), (b"zyx", 1), (b"q", 0), (b"yzx", 2)):
        out.append(Case("x?y?z? on %r" % head, XYZ, _with(filler(79, n) if head != b"q" else np.full(n, ord("q"), np.uint8), 0, head), (0, e)))
    return out


def url_cases():
    """Large tables whose chunk maps converge: URLs planted with their ends at the forward grid's first edges; a look-alike without
    a top-level domain in front."""
    out, n = [], 256 * 300 + 40
    p = url_pattern()
    fill = np.frombuffer(b" \n!*", dtype=np.uint8)                # (z and q are path characters)
    for s, total in ((0, 255), (0, 256), (0, 257), (256 * 150 - 5, 256 + 3840 + 1), (n - 300, 300)):
        head = b"https://ab-1.example.com:8080/"
        body = np.frombuffer(b"abcXYZ019._~%-/", dtype=np.uint8)[np.random.default_rng(total).integers(0, 15, size=total - len(head))]
        t = filler(83 + total, n, fill)
        if s >= 40:
            plant(t, s - 30, b"http://nodomain/ ftp:/x.yz")
        plant(t, s, np.concatenate([_arr(head), body]))
        out.append(Case("url at %d, %d bytes" % (s, total), p, t, (s, s + total)))
    out.append(Case("url none", p, _with(filler(89, n, fill), 1000, b"http://nodomain/ ftp:/x.yz"), NONE))
    return out


ODD_OFFSETS = (1, 7, 16)


def odd_address_cases():
    """The string at an address = 1, 7, 16 mod 16: the backward pass' single bytes down to an aligned address, the forward pass'
    first window (255, 249, 256 bytes) - matches that end at that hand-over and one byte to either side."""
    out, n = [], 256 * 300 + 16 + 3
    for skew in ODD_OFFSETS:
        first = FIRST_WINDOW - (skew & 15)
        for d in (first - 1, first, first + 1, first * (WINDOW_GROWTH + 1), 256 * 131):
            out.append(Case("odd address %d number end at +%d" % (skew, d), NUMBER, number_text(n, 0, d, 97 + d % 31), (0, d), skew=skew))
        length = 2 + 5 * ((n - 600) // 5)
        out.append(Case("odd address %d W(5)" % skew, W(5), w_text(5, n, 301, length, 101 + skew), (301, 301 + length), skew=skew))
        out.append(Case("odd address %d W(5) none" % skew, W(5), _with(filler(103, n), 301, w_run(5, length - 1, 5)), NONE, skew=skew))
    return out


def domain_cases():
    """A NUL and a byte >= 0x80 INSIDE what would be a match - in the first 64 bytes that the backward pass walks of a chunk, in the
    chunk's rest, as the last byte it walks: no match there, the second true match further right is the answer.  (Outside the
    matches every filler has them.)"""
    out, n, k = [], 256 * 300 + 40, 5
    length = 2 + k * 8000
    s = 256 * 20 + 9
    good = w_text(k, n, s, length, 107)
    second = closed_w(k, good[s + length:])
    assert second != NONE
    second = (second[0] + s + length, second[1] + s + length)
    out.append(Case("domain clean", W(k), good, (s, s + length)))
    edge = n - 256 * 150                                      # a chunk boundary of the backward grid, inside the match
    assert s < edge - 256 and edge < s + length
    for name, pos in (("prefix of a chunk", edge - 5), ("rest of a chunk", edge - 256 + 9), ("last byte of a chunk", edge - 256)):
        for bad in (0x00, 0xC3):
            t = good.copy()
            t[pos] = bad
            out.append(Case("domain 0x%02x in the %s" % (bad, name), W(k), t, second))
    t = t.copy()
    t[second[0] + 3] = 0x00                                   # ... and in the second match too: none
    out.append(Case("domain: both matches broken", W(k), t, NONE))
    return out


THREE_LEVELS = L.THREE_LEVELS        # 1024 * 16384 + 1 bytes: backwards 16385 chunks of 1 KiB, 129 groups, 2 at level 2


@functools.lru_cache(maxsize=None)
def three_level_cases():
    """The W(5) match runs from the FIRST byte - the one-byte chunk that the backward pass walks last, entered through all three
    levels in a live state - to 64 bytes before the end; the variant's run is one byte longer: the small match planted behind it
    is the answer."""
    n, tail = THREE_LEVELS, 64
    nab = 5 * ((n - tail - 2) // 5)
    out = []
    for extra, name in ((0, "whole-string match"), (1, "run one byte longer")):
        t = filler(109, n)
        plant(t, 0, w_run(5, nab + extra, 113))
        small = nab + extra + 2 + 7
        plant(t, small, w_run(5, 10, 127))
        out.append(Case("three levels W(5), %s" % name, W(5), t, (small, small + 12) if extra else (0, nab + 2)))
    return out


# Forwards the windows from an aligned start are 256, 3840, 61440, 983040 and 15728640 bytes - 16 MiB walked - and the sixth takes
# what is left, up to 240 MiB: with 1024 * 16384 + 69 bytes left it has 16385 chunks of 1 KiB, 129 groups, 2 at level 2.
FORWARD_WALKED = 16 << 20
FORWARD_THREE_LEVELS = FORWARD_WALKED + 1024 * 16384 + 69


@functools.lru_cache(maxsize=None)
def forward_three_level_cases():
    """The W(5) match runs from byte 0 into the LAST chunk of the sixth forward window (69 bytes, entered through all three levels in
    a live state) and ends 64 bytes before the string does; the variant's run is one byte longer: the small match planted behind
    it, in the same chunk, is the answer.  (Backwards the string has 32769 chunks: three levels there too.)"""
    n, tail = FORWARD_THREE_LEVELS, 64
    nab = n - tail - 2
    assert nab % 5 == 0 and forward_windows(0, n)[-1] == (FORWARD_WALKED, n - FORWARD_WALKED) and len(forward_windows(0, n)) == 6
    assert long_chunk(n - FORWARD_WALKED) == 1024 and nab + 2 > FORWARD_WALKED + 1024 * 16384
    out = []
    for extra, name in ((0, "whole-string match"), (1, "run one byte longer")):
        t = filler(131, n)
        plant(t, 0, w_run(5, nab + extra, 137))
        small = nab + extra + 2 + 7
        plant(t, small, w_run(5, 10, 139))
        out.append(Case("forward three levels W(5), %s" % name, W(5), t, (small, small + 12) if extra else (0, nab + 2)))
    return out


SET_NAMES = ("number positions", "W(5) positions", "W(7) positions", "geometry", "slots and rotation", "start cases", "hand-over", "nullable",
             "url", "odd addresses", "domain")


@functools.lru_cache(maxsize=None)
def small_case_sets():
    """name -> cases, every set but the 16 MiB pair, built once per process and never changed (the device test takes each under its
    name)."""
    sets = {"number positions": number_position_cases(), "W(5) positions": w_position_cases(5), "W(7) positions": w_position_cases(7),
            "geometry": geometry_cases(), "slots and rotation": slot_cases(), "start cases": start_cases(), "hand-over": handover_cases(),
            "nullable": nullable_cases(), "url": url_cases(), "odd addresses": odd_address_cases(), "domain": domain_cases()}
    assert tuple(sets) == SET_NAMES
    return sets
