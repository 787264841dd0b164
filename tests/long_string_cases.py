"""Pattern families, references and case sets for rrx_match_string (one long string: kernels_long.hip, long_rows_nfa_kernel).
Shared by test_match_string_lowering.py (CPU) and test_match_string_gpu.py (device).  Test infrastructure only.

The families have chunk maps that neither converge nor commute, so that the ORDER in which chunk maps are composed, a chunk
taken twice or not at all, and a level read from the wrong place all change the verdict:

  P3   = (b|a(a|b)(b(a|b))*a)*  over {a, b}: the 3-state automaton of the dihedral group of order 6 - `a` maps state i to
         i + 1 mod 3, `b` maps i to -i mod 3; start 0, which alone accepts.
  Z(k) = ((a|b){k})*            k live states on a cycle (the maps are rotations: they commute, but they never converge).
  U(k) = cP3|cZ(k)              a `c`, then text accepted by P3 or by Z(k).  The table is the product of the two (3k live
         states, the start and the dead row: D = 3k + 2, NFA positions k + 9), its maps do not commute; k chooses D / nbits.
         NOT written P3|Z(k): in the reference's dialect a starred alternative falls through into the next one
         (`x*|y*` accepts `xxyy`; the oracle and Python's re disagree on it), so P3|Z(k) is P3 FOLLOWED BY Z(k), which accepts
         nearly every long random string.  With the `c` in front neither alternative is nullable and the union is the union.
  R(k) = (((a|b){k})*c)*((a|b){k})*   a `c` sends residue 0 to the start and everything else to the dead state: a chunk with a
         `c` in its first 64 bytes keeps 2 distinct prefix states, a chunk without one k + 1.

Closed forms (numpy) give the references for strings the oracle would take long on; the CPU file pins them to the oracle.
The chunk-composition MODEL restates what match_long_dfa / match_long_nfa assemble from a DfaReplay of the plain table -
chunk maps, then groups of `group` maps composed level by level - and can be run with one named mutation."""
import numpy as np

P3 = "(b|a(a|b)(b(a|b))*a)*"
A, B, C_ = ord("a"), ord("b"), ord("c")

K_LONG_GROUP = 128          # device.hpp kLongGroup
K_LONG_SLOTS = 4            # kernels_long.hip kLongSlots
K_LONG_PREFIX = 64          # kernels_long.hip kLongPrefix
K_LONG_MAX_STATES = 254     # device.hpp kLongMaxStates
TABLE_FROM = 1024           # strings.cpp kLongStringBytesTable
NFA_FROM = 32 * 1024        # strings.cpp kLongStringBytes
NFA_MAX_BITS = 256          # strings.cpp kLongNfaMaxBits


def Z(k):
    return "((a|b){%d})*" % k


def U(k):
    return "c" + P3 + "|c" + Z(k)


def R(k):
    return "(((a|b){%d})*c)*((a|b){%d})*" % (k, k)


# U(k) per regime of per_block = 256 / D on the table path (D = 3k + 2 read from the dump: test_match_string_lowering.py)
K_BLOCK = {"D<=85": 27, "D 86..128": 42, "D 129..253": 43, "D=254": 84, "D>=255": 85}
# U(k) per width of the NFA program (nbits = k + 9; W as dumped -> the width the kernel is instantiated at)
K_WIDTH = {2: 40, 3: 70, 4: 100, 5: 130, 6: 170, 7: 200, 8: 230}
K_NFA_FALLBACK = 250        # nbits 259 > 256: one lane


# ------------------------------------------------------------------------------------------------ closed forms
def _arr(s):
    return np.frombuffer(s, dtype=np.uint8) if isinstance(s, (bytes, bytearray)) else np.asarray(s, dtype=np.uint8)


def p3_state(s):
    """State of P3 after the a/b text s: sum over the a-positions of (-1)^(number of b after it), mod 3."""
    s = _arr(s)
    if s.size == 0:
        return 0
    isb = (s == B).astype(np.int64)
    after = isb[::-1].cumsum()[::-1] - isb            # b's strictly after each position
    sign = 1 - 2 * (after & 1)
    return int(sign[s == A].sum() % 3)


def _is_ab(s):
    return bool(((s == A) | (s == B)).all())


def accepts_p3(s):
    s = _arr(s)
    return _is_ab(s) and p3_state(s) == 0


def accepts_z(k, s):
    s = _arr(s)
    return _is_ab(s) and s.size % k == 0


def accepts_u(k, s):
    s = _arr(s)
    if s.size == 0 or s[0] != C_ or not _is_ab(s[1:]):
        return False
    return (s.size - 1) % k == 0 or p3_state(s[1:]) == 0


def accepts_r(k, s):
    s = _arr(s)
    if not bool(((s == A) | (s == B) | (s == C_)).all()):
        return False
    cut = np.concatenate([[-1], np.nonzero(s == C_)[0], [s.size]])
    return bool(((np.diff(cut) - 1) % k == 0).all())


def reference(family, k=None):
    """family: 'P3' | 'Z' | 'U' | 'R' -> (pattern, closed form)"""
    if family == "P3":
        return P3, accepts_p3
    pat = {"Z": Z, "U": U, "R": R}[family](k)
    fn = {"Z": accepts_z, "U": accepts_u, "R": accepts_r}[family]
    return pat, (lambda s, fn=fn, k=k: fn(k, s))


# ------------------------------------------------------------------------------------------------ the model
def long_chunk(nbytes):
    """kernels_long.hip long_chunk"""
    chunk = 256
    while (nbytes + chunk - 1) // chunk > (1024 if chunk < 1024 else 65536):
        chunk <<= 1
    return chunk


def nfa_chunk(nbytes, nbits, W):
    """kernels_coop.hip long_nfa_scratch_bytes"""
    c, per_chunk = 1024, nbits * W * 4
    while (nbytes + c - 1) // c > 65536 or ((nbytes + c - 1) // c) * per_chunk > (256 << 20):
        c <<= 1
    return c


def chunk_maps(d, data, chunk, limit=None):
    """maps[k][s] = state after (the first `limit` bytes of) chunk k from state s, as long_maps_kernel builds them: a byte
    >= 0x80 takes the column of 128."""
    a = _arr(data)
    col = np.asarray(d.cls, dtype=np.int64)[np.minimum(a, 128)]
    nxt = np.asarray(d.next, dtype=np.int64)
    n, full = (a.size + chunk - 1) // chunk, a.size // chunk
    maps = np.tile(np.arange(d.nstates, dtype=np.int64), (n, 1))
    body = col[:full * chunk].reshape(full, chunk)
    for j in range(chunk if limit is None else min(limit, chunk)):
        maps[:full] = nxt[maps[:full], body[:, j][:, None]]
    tail = col[full * chunk:]
    for c in (tail if limit is None else tail[:limit]):
        maps[full] = nxt[maps[full], c]
    return maps


def prefix_distinct(d, data, chunk):
    """Per chunk the number of distinct states after its first 64 bytes (step A): <= 4 takes the slots, more is flagged."""
    pre = chunk_maps(d, data, chunk, limit=K_LONG_PREFIX)
    return np.array([np.unique(row).size for row in pre])


MUTATIONS = ("swap_chunks", "reverse_order", "drop_last", "first_twice", "next_group")


def compose(maps, group=K_LONG_GROUP, mutation=None, spare_last=False):
    """The levels of long_compose_kernel (group 128) / long_compose_nfa_kernel (group 2: a last odd one is copied):
    out[g] = in[g*group + group-1] o ... o in[g*group], until one map is left.  Mutations, applied to every group of every
    level that has at least two members: swap_chunks (the two middle members change places), reverse_order (composed last to
    first), drop_last (the last member is left out), first_twice (the first member is applied twice); next_group: at level 2
    group g is composed from the members of group g + 1 (where there is one).  spare_last: the last group of every level - the
    one that holds the end of the string - is composed faithfully, the defect sits in the others alone."""
    assert mutation is None or mutation in MUTATIONS
    cur, lvl = maps, 0
    ident = np.arange(maps.shape[1], dtype=np.int64)
    while len(cur) > 1:
        lvl += 1
        m = (len(cur) + group - 1) // group
        out = np.empty((m, maps.shape[1]), dtype=np.int64)
        for g in range(m):
            src = g + 1 if (mutation == "next_group" and lvl == 2 and g + 1 < m) else g
            seq = list(range(src * group, min((src + 1) * group, len(cur))))
            if len(seq) >= 2 and not (spare_last and g == m - 1):
                if mutation == "swap_chunks":
                    h = len(seq) // 2
                    seq[h - 1], seq[h] = seq[h], seq[h - 1]
                elif mutation == "reverse_order":
                    seq.reverse()
                elif mutation == "drop_last":
                    seq.pop()
                elif mutation == "first_twice":
                    seq.insert(0, seq[0])
            s = ident
            for k in seq:
                s = cur[k][s]
            out[g] = s
        cur = out
    return cur[0]


def model_verdict(d, maps, group=K_LONG_GROUP, mutation=None, spare_last=False):
    return bool(d.acc[compose(maps, group, mutation, spare_last)[d.start]])


# ------------------------------------------------------------------------------------------------ strings
def ab(seed, n):
    return np.frombuffer(b"ab", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 2, size=n)]


def text_for(family, seed, n):
    """A random string of n bytes in the family's domain (U: a `c`, then a/b)."""
    t = ab(seed, n)
    if family == "U":
        t = t.copy()
        t[0] = C_
    return t


def both_verdicts(family, k, n, seed):
    """Two strings of n bytes, the first accepted and the second rejected: seeds seed, seed + 1, ... until both are there."""
    _, fn = reference(family, k)
    got = {}
    for s in range(seed, seed + 200):
        t = text_for(family, s, n)
        got.setdefault(fn(t), (s, t))
        if len(got) == 2:
            return [got[True], got[False]]
    raise AssertionError(("one verdict only", family, k, n))


class Case:
    """One string of a device test: `pattern` on `data` has to give `want`; `tag` names it in messages."""

    def __init__(self, tag, family, k, data, want=None):
        self.tag, self.family, self.k, self.data = tag, family, k, np.ascontiguousarray(data, dtype=np.uint8)
        self.pattern, fn = reference(family, k)
        self.want = fn(self.data) if want is None else want

    def __repr__(self):
        return "%s[%d bytes]" % (self.tag, self.data.size)


def _pairs(prefix, family, k, lengths, seed):
    out = []
    for n in lengths:
        for s, t in both_verdicts(family, k, n, seed + n % 1000):
            out.append(Case("%s n=%d seed=%d" % (prefix, n, s), family, k, t))
    return out


# ---- table path, geometry: the 1 KiB threshold; 256-byte chunks at one and two levels, a last chunk of one byte, the
# 1024-chunk limit of the 256-byte regime; the chunk size changing at 256 KiB; 384 chunks of 1 KiB + 7
GEOMETRY_LENGTHS = ((1023, 1024, 1025) + tuple(256 * n + r for n in (127, 128, 129, 1024) for r in (0, 1, 255))
                    + (256 * 1024 - 1, 256 * 1024, 256 * 1024 + 1, 1024 * 128 * 3 + 7))
GEOMETRY_K = 5                                  # U(5): D = 17, per_block 15; no length here has (n - 1) % 5 == 0
THREE_LEVELS = 1024 * 16384 + 1                 # the smallest length with more than 128^2 chunks (of 1 KiB)
THREE_LEVELS_SEED = 1                           # chosen so that `next_group` flips it (test_match_string_lowering.py)


def geometry_cases(family):
    return _pairs("geometry %s" % family, family, GEOMETRY_K if family == "U" else None, GEOMETRY_LENGTHS, 100)


def three_level_case():
    return Case("three levels P3 seed=%d" % THREE_LEVELS_SEED, "P3", None, ab(THREE_LEVELS_SEED, THREE_LEVELS))


# ---- table path, slots
# 130, 141, 201, 256 chunks of 256 bytes: two levels; n - 1 is a multiple of no k used with them (U(k) would accept every string)
TWO_LEVEL_LENGTHS = (256 * 129 + 2, 256 * 140 + 9, 256 * 200 + 77, 64 * 1024 - 5)


def rotation_cases(k):
    """Z(k): every chunk keeps k + 1 > 4 distinct prefix states and is stepped from every state (step A')."""
    out = []
    for n in TWO_LEVEL_LENGTHS:
        lo = n - n % k
        for m in (lo, lo + 1, n + k - n % k):
            out.append(Case("rotation Z(%d) n=%d" % (k, m), "Z", k, ab(7 * k + m % 97, m)))
    return out


def reset_cases(k):
    """R(k), `c` placed by construction: chunks 0, 3, 6, ... have a `c` in their first 64 bytes (2 distinct prefix states: the
    slots), every fifth chunk has one in its rest, the others none (k + 1 distinct: flagged) - so the batches of 256 / D chunks
    of step A' mix flagged and unflagged chunks.  Accepted: every segment a multiple of k; rejected: one `c` moved by one byte,
    in an early chunk, in the middle and in the last chunk."""
    nchunks, chunk = 300, 256
    at, last = [], -1
    for j in range(nchunks):
        for lo in ((chunk * j,) if j % 3 == 0 else ()) + ((chunk * j + 100,) if j % 5 == 0 else ()):
            p = lo + (last + 1 - lo) % k           # the first p >= lo with (p - last - 1) % k == 0
            assert p > last and p - lo < k
            at.append(p)
            last = p
    n = at[-1] + 1 + 3 * k
    assert long_chunk(n) == chunk and K_LONG_GROUP < n // chunk == at[-1] // chunk      # two levels; a `c` in the last chunk
    good = ab(11 * k, n).copy()
    good[at] = C_
    out = [Case("reset R(%d) accepted" % k, "R", k, good)]
    for name, i in (("early", 1), ("middle", len(at) // 2), ("last chunk", len(at) - 1)):
        t = good.copy()
        t[at[i]], t[at[i] + 1] = t[at[i] + 1], C_
        assert t[at[i]] != C_
        out.append(Case("reset R(%d) %s c moved to %d" % (k, name, at[i] + 1), "R", k, t))
    return out


# ---- table path, per_block = 256 / D: 3 and more, 2, 1, the largest admitted table, and the hand-over to the one-item path
def per_block_cases(regime):
    k = K_BLOCK[regime]
    return _pairs("per_block U(%d)" % k, "U", k, TWO_LEVEL_LENGTHS, 300 + k)


# ---- bytes outside the domain: NUL and a byte >= 0x80, in the first 64 bytes of a middle chunk, in its rest, as last byte
def domain_cases(family, k, n, chunk):
    (_, good), _ = both_verdicts(family, k, n, 500)
    mid = chunk * ((n // chunk) // 2)
    out = [Case("domain %s n=%d clean" % (family, n), family, k, good)]
    for name, pos in (("prefix of a middle chunk", mid + 5), ("rest of a middle chunk", mid + chunk - 9), ("last byte", n - 1)):
        for bad in (0x00, 0xC3):
            t = good.copy()
            t[pos] = bad
            out.append(Case("domain %s n=%d 0x%02x in the %s" % (family, n, bad, name), family, k, t, want=False))
    return out


DOMAIN_TABLE_N = 256 * 300 + 40
DOMAIN_NFA_N = 35 * 1024 - 100


# ---- NFA path: 32 KiB - 1 stays on one lane; 32, 33 and 35 chunks of 1 KiB (33 is odd at every level: 33, 17, 9, 5, 3, 2)
NFA_LENGTHS = (32 * 1024 - 1, 32 * 1024, 32 * 1024 + 1, 33 * 1024 - 5, 35 * 1024 - 100)


def nfa_cases(family, k):
    return _pairs("nfa %s%s" % (family, "" if k is None else "(%d)" % k), family, k, NFA_LENGTHS, 700 + (k or 0))


# ---- a string at an odd address: dev[1:], dev[7:], dev[16:] of one buffer
ODD_OFFSETS = (1, 7, 16)
ODD_BUFFER_N = 256 * 300 + 16 + 3               # 301 chunks of 256 bytes (two levels); 76 chunks of 1 KiB on the NFA path


def odd_address_buffer():
    """One a/b buffer whose three slices hold both verdicts."""
    for seed in range(900, 1100):
        buf = ab(seed, ODD_BUFFER_N)
        if len({accepts_p3(buf[o:]) for o in ODD_OFFSETS}) == 2:
            return seed, buf
    raise AssertionError("no buffer with both verdicts")
