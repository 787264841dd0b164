"""The case table of the three cooperative NFA engines: the group-cooperative kernels (kernels_coop.hip: GroupNfa<G, K, MODE, SLOT0>,
8 geometries x 3 builds), the wave-resident kernels (kernels_wave.hip: WaveNfa<WL, FRONT>) and the sparse kernels (SparseNfa<WR,
LROWS>) - every instantiation the front end can reach, with the lines each case runs on and a CLOSED FORM of its language as the
reference.  Shared by test_coop_engines_lowering.py (no GPU: which instantiation a case reaches, the replays, the mutants) and
test_coop_engines_gpu.py (the kernels on the same lines).  Needs neither a GPU nor torch.

The oracle cannot be the reference at these sizes (it walks the reference automaton's edge lists: minutes per text at 28 000
positions); every closed form is held against it at a small member of its family (SMALL) by the lowering test.

    family   pattern                                 positions   group build                        wave / sparse
    carry3   (a|b)*a(a|b){n}                         n + 3       <2, true>                          FRONT, exceptions
    bstar    b*a{1,n}                                n + 2       <2, false>                         FRONT, exceptions
    chain1   a{1,n}                                  n + 1       <0, false>: no self, no exception  FRONT, no exception
    chainx   a{n}                                    n + 1       -                                  FRONT, no exception
    selfhi   a{n}b*                                  n + 2       <0, false>: self in a high slot    !FRONT by the self term
    exc      (ab|ba){1,k}                            4k + 2      <0, false>: exceptions everywhere  !FRONT by exceptions
    star     ((a|b)*a(a|b){m}c|(b|c)*b(b|c){m'}a)*   m + m' + 7  <0, false>: edges across lanes     (reference: the oracle)
    heads    h1?h2?...hj?a{n}                        n + j + 1   -                                  sparse: j + 2 byte classes
    segs     a{n1}b{n2}...g{n7}                      sum + 1     -                                  sparse: 8 byte classes at 32 769 positions
"""
import random
from collections import namedtuple

ENGINE_NFA_WAVE, ENGINE_NFA_BLOCK, ENGINE_NFA_SPARSE = 4, 8, 10       # (roaringregex_amd's constants: the lowering test compares)
ENGINE_OF = {"group": ENGINE_NFA_WAVE, "wave": ENGINE_NFA_BLOCK, "sparse": ENGINE_NFA_SPARSE}
ENGINE_NAME = {"group": "nfa-group-cooperative", "wave": "nfa-wave-resident", "sparse": "nfa-wave-sparse"}

# inst: ("group", G, K, MODE, SLOT0) / ("wave", WL, FRONT) / ("sparse", WR, LROWS); edge: "full" (nbits == the form's capacity), "low"
# (the smallest nbits that selects it) or ""
Case = namedtuple("Case", "id engine family pattern n nbits inst edge")

GROUP_FORMS = ((8, 3), (8, 4), (16, 3), (16, 4), (32, 3), (32, 4), (32, 5), (32, 8))           # device.hpp: group_geometry
GROUP_BUILDS = ((0, False), (2, False), (2, True))                                             # kernels_coop.hip: RRX_GROUP_FORM
WAVE_WIDTHS = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32)                                               # kernels_wave.hip: wave_words_per_lane
SPARSE_ROWS = (1, 2, 4, 8, 16, 32)                                                             # kernels_wave.hip: sparse_rows
SPARSE_LDS_BUDGET = 48 * 1024                                                                  # kernels_wave.hip: kSparseRowsLdsBudget
GROUP_MIN_BITS = 513                                                                           # AUTO's first size beyond the lane engine
MAX_CLASSES = 128                                                                              # 0x00 and >= 0x80 share class 0 with every unused byte


def group_geometry(nbits):
    for G, K in GROUP_FORMS:
        if nbits <= 32 * G * K:
            return G, K
    return None


def wave_words_per_lane(words):
    need = (words + 63) // 64
    return next((w for w in WAVE_WIDTHS if need <= w), 0)


def sparse_rows(words):
    need = (words + 63) // 64
    return next((w for w in SPARSE_ROWS if need <= w), 0)


# What the front end cannot reach (it refuses more than 65 536 reference states, and the reference spends two states on every
# position: test_coop_engines_lowering.py asserts the refusals at the smallest sizes that would select it): WL 32 needs 49 153
# positions; 32 769 are the most there are - which is where WR 32 begins (the sparse form has no 24 rows), so that one IS reached.
# SparseNfa<1, false> needs 193 byte classes (ncls x WR x 256 bytes > 48 KiB); there are 128 at most.
UNREACHABLE = {("wave", 32, True), ("wave", 32, False), ("sparse", 1, False)}
REACHABLE = ({("group", G, K, m, s) for G, K in GROUP_FORMS for m, s in GROUP_BUILDS} |
             {("wave", WL, f) for WL in WAVE_WIDTHS for f in (True, False) if (WL, f) != (1, False)} |
             {("sparse", WR, l) for WR in SPARSE_ROWS for l in (True, False)}) - UNREACHABLE
# (WaveNfa<1, false> is compiled and never chosen: with one word per lane every word is word 0)

# head bytes of the many-class family: everything below 0x80 that the pattern syntax leaves alone, but ' ' (kept outside every class)
_SPECIAL = set(b"\\.[](){}|*+?^$-\n a")
HEAD_BYTES = [c for c in range(1, 128) if c not in _SPECIAL]


def _heads(j):
    return bytes(HEAD_BYTES[:j])


def _pairs(rng, j):
    return b"".join(rng.choice((b"ab", b"ba")) for _ in range(j))


def _ab(rng, L):
    return bytes(rng.choice(b"ab") for _ in range(L))


def _units(t):
    """number of ab / ba units of t, or -1"""
    if len(t) % 2 or any(t[i:i + 2] not in (b"ab", b"ba") for i in range(0, len(t), 2)):
        return -1
    return len(t) // 2


def _heads_form(t, n, j):
    H, i = _heads(j), 0
    body = t.rstrip(b"a")
    if len(t) - len(body) < n:
        return False
    body += b"a" * (len(t) - len(body) - n)                  # ('a' is no head: anything left in front of a^n has to be heads in order)
    for c in body:
        while i < len(H) and H[i] != c:
            i += 1
        if i == len(H):
            return False
        i += 1
    return True


# family, parameter -> (pattern, positions, closed form: line -> bool, or None = the oracle, a byte outside the classes)
def _fam(family, n):
    if family == "carry3":
        return ("(a|b)*a(a|b){%d}" % n, n + 3, lambda t: len(t) >= n + 1 and not t.strip(b"ab") and t[len(t) - n - 1] == 97, b"c")
    if family == "bstar":
        return ("b*a{1,%d}" % n, n + 2, lambda t: not t.strip(b"ab") and b"ab" not in t and 1 <= t.count(b"a") <= n, b"c")
    if family == "chain1":
        return ("a{1,%d}" % n, n + 1, lambda t: 1 <= len(t) <= n and not t.strip(b"a"), b"c")
    if family == "chainx":
        return ("a{%d}" % n, n + 1, lambda t: len(t) == n and not t.strip(b"a"), b"c")
    if family == "selfhi":
        return ("a{%d}b*" % n, n + 2, lambda t: t[:n] == b"a" * n and not t[n:].strip(b"b"), b"c")
    if family == "exc":
        return ("(ab|ba){1,%d}" % n, 4 * n + 2, lambda t: 1 <= _units(t) <= n, b"c")
    if family == "star":
        m, m2 = n
        return ("((a|b)*a(a|b){%d}c|(b|c)*b(b|c){%d}a)*" % (m, m2), m + m2 + 7, None, b"d")
    if family == "segs":                                     # one run per letter: a class per run, two reference states per position
        member = b"".join(bytes([97 + i]) * k for i, k in enumerate(n))
        return ("".join("%s{%d}" % (chr(97 + i), k) for i, k in enumerate(n)), sum(n) + 1, lambda t: t == member, bytes([97 + len(n)]))
    j, k = n                                                 # heads: j optional heads, then a{k}
    return ((b"".join(bytes([c]) + b"?" for c in _heads(j)) + b"a{%d}" % k).decode("latin-1"), k + j + 1, lambda t: _heads_form(t, k, j), b" ")


def pattern_of(family, n):
    return _fam(family, n)[0]


def positions(family, n):
    return _fam(family, n)[1]


def accepts(case_or_family, t, n=None):
    """the closed form's verdict on one line (bytes)"""
    family, n = (case_or_family.family, case_or_family.n) if n is None else (case_or_family, n)
    return bool(_fam(family, n)[2](t))


SMALL = {"carry3": 37, "bstar": 70, "chain1": 75, "chainx": 75, "selfhi": 70, "exc": 17, "heads": (14, 60), "segs": (9, 9, 8, 8, 8, 8, 7)}    # each confirmed by the oracle


def _boundaries(inst, nbits):
    """positions at which a carry leaves one lane (row) of the layout for the next: a few of them, the DPP row boundary of a 32-lane
    group among them"""
    if inst[0] == "group":
        G, K = inst[1], inst[2]
        step, picks = 32 * K, (1, 2, 15, 16, 17, G - 1)
    elif inst[0] == "wave":
        step, picks = 32 * inst[1], (1, 2, 32, 63)
    else:
        step, picks = 2048, (1, 2, inst[1] - 1)
    return sorted({step * l for l in picks if 0 < step * l < nbits})


def _around(ps, lo, hi):
    return sorted({L for p in ps for L in (p - 1, p, p + 1) if lo <= L <= hi})


def _lane_lengths(inst, nbits, lo, hi):
    """lengths at which the live position of a chain sits on a lane boundary: EVERY lane of a group (every eighth lane of the wave's 64)
    exactly, the picked ones of _boundaries one to either side as well"""
    step, lanes = (32 * inst[2], range(1, inst[1])) if inst[0] == "group" else (32 * inst[1], range(8, 64, 8)) if inst[0] == "wave" else (2048, ())
    return sorted(set(_around(_boundaries(inst, nbits), lo, hi)) | {step * l for l in lanes if lo <= step * l <= hi and step * l < nbits})


def _family_lines(family, n, inst, rng):
    """members and near misses of the family at this size: the accept edges n - 1, n, n + 1, lengths around the layout's lane
    boundaries, a byte outside the classes late in a long line and while the live position sits in a slot above 0, one wrong letter"""
    nbits, out_c = positions(family, n), _fam(family, n)[3]
    E = _boundaries(inst, nbits)
    a, b = b"a", b"b"
    if family in ("chain1", "chainx"):
        out = [a * L for L in [1, 2, n - 1, n, n + 1, n + 2] + (_lane_lengths(inst, nbits, 1, n) if family == "chain1" else [])]
        out += [a * (n - 1) + b, b + a * (n - 1), a * 40 + b + a * 3, a * 40 + out_c + a * 3, a * (n - 2) + out_c + a, a * (n - 2) + b"\x00" + a,
                a * (n - 2) + b"\x80" + a, a * (n // 2) + b + a * (n - n // 2 - 1)]
        return out
    if family == "bstar":
        out = [b * j + a * L for j in (0, 1, 3) for L in (0, 1, n - 1, n, n + 1)] + [b + a * (L - 1) for L in _lane_lengths(inst, nbits, 2, n)]
        out += [b * 2 + a * (n - 1) + b, a * (n - 1) + b + a, a + b + a * (n - 2), b + a * 40 + b + a * 3, b + a * 40 + out_c + a * 3,
                b + a * (n - 3) + out_c + a, b + a * (n - 3) + b"\x00" + a, b + a * (n - 3) + b"\x80" + a]
        return out
    if family == "selfhi":
        out = [a * n + b * j for j in (0, 1, 2, 40)] + [a * (n - 1), a * (n + 1), a * (n - 1) + b, a * (n - 1) + b * 2, a * n + b + a, a * n + b * 3 + a, b + a * n]
        out += [a * 40 + b + a * (n - 41) + b, a * 40 + out_c + a * (n - 41) + b, a * n + b + out_c + b, a * n + b"\x00" + b, a * n + b * 2 + b"\x80",
                a * (n // 2) + b + a * (n - n // 2)]
        return out
    if family == "carry3":
        out = []
        for lead in (0, 1, 50):
            out += [b * lead + a + b * n, b * lead + b + b * n, a * lead + a + a * n, b * lead + a + b * (n + 1)]
        out += [_ab(rng, 7) + a + _ab(rng, n), _ab(rng, 7) + b + _ab(rng, n), a * n, b + a * n, b * (n + 1), a + b * (n - 1)]
        # (the mark's bit walks through every lane whatever the lead: the set itself is what sits on the boundaries - two marks that
        # far apart, the one that decides and one that does not)
        out += [a + b * (p - 1) + a + b * (n - p) for p in _around(E, 2, n - 1)[:9]] + [b + b * (p - 1) + a + b * (n - p) for p in E[:3]]
        out += [b + a + b * 40 + out_c + b * (n - 41), b + a + b * (n - 4) + out_c + b * 3, b + a + b * (n - 4) + b"\x00" + b * 3,
                a + b * (n - 4) + b"\x80" + b * 3, a + b * 40 + b"\x80" + b * (n - 41)]
        return out
    if family == "exc":
        k = n
        out = []
        for j in (0, 1, 2, k - 1, k, k + 1):
            out += [_pairs(rng, j), b"ab" * j, b"ba" * j]
        out += [_pairs(rng, k), _pairs(rng, k - 1) + b"aa", _pairs(rng, k - 1) + b"bb", _pairs(rng, k)[:-1], _pairs(rng, k) + a, a + _pairs(rng, k - 1) + b]
        out += [_pairs(rng, L // 4) for L in _around(E, 8, 4 * k)[1::3]]
        out += [_pairs(rng, 10) + out_c + _pairs(rng, k - 11), _pairs(rng, 10) + b"aa" + _pairs(rng, k - 11), _pairs(rng, 11) + b"b" + _pairs(rng, k - 12),
                _pairs(rng, 10) + b"a" + out_c + _pairs(rng, k - 11), _pairs(rng, k - 2) + out_c + _pairs(rng, 1), _pairs(rng, k - 2) + b"\x00" + _pairs(rng, 1),
                _pairs(rng, k - 2) + b"\x80" + _pairs(rng, 1)]
        return out
    if family == "star":
        m, m2 = n

        def u1(lead=0):
            return _ab(rng, lead) + a + _ab(rng, m) + b"c"

        def u2(lead=0):
            return bytes(rng.choice(b"bc") for _ in range(lead)) + b + bytes(rng.choice(b"bc") for _ in range(m2)) + a
        out = [b"", u1(), u2(), u1(3), u2(5), u1() + u2(), u2() + u1(), u1(2) + u1(), u1(4) + u2(1), u1()[:-1], u2()[:-1], u1() + b"c", u2() + a + a, u2() + b"c", u2(2) + b"cc",
               b"c", a, a * (m + 1) + b"c", b * (m2 + 1) + a, b * (m2 + 1), u1()[1:], b"c" + u2(), u1() + out_c, u1(1)[:m] + out_c + b"c" * 2, u1() + u2()[:-3] + b"\x80" + a * 2]
        return out
    if family == "segs":
        M = b"".join(bytes([97 + i]) * k for i, k in enumerate(n))
        last = M[-1:]
        out = [M, M[:-1], M + last, M + out_c, M[:-3] + out_c + M[-2:], M[:-3] + b"\x00" + M[-2:], M[:-3] + b"\x80" + M[-2:], M[:40] + out_c + M[41:], M[1:]]
        cuts = [sum(n[:i]) for i in range(1, len(n))]
        out += [M[:p - 1] + M[p:p + 1] + M[p:] for p in cuts[:2]] + [M[:p] + M[p - 1:p] + M[p + 1:] for p in cuts[:2] + cuts[-1:]]     # a run ends early / late
        out += [M[:p] + out_c + M[p + 1:] for p in _around(E[:2], 1, len(M) - 1)]
        return out
    j, k = n                                                 # heads
    H = _heads(j)
    out = [H[::3] + a * k, H + a * k, a * k, H[:1] + a * k, H[-1:] + a * k, H[::2] + a * (k - 1), H[::2] + a * (k + 1), a * (k - 1), a * (k + 1),
           H[1:2] + H[:1] + a * k, H[:3] + H[:1] + a * k, H[:2] + a * 5 + H[3:4] + a * (k - 5), H[:2] + a * (k - 3) + out_c + a * 3,
           a * (k - 3) + b"\x00" + a * 3, H[-2:] + a * (k - 3) + b"\x80" + a * 3, a * (k // 2) + out_c + a * (k - k // 2)]
    out += [H[:5] + a * (L - 5) for L in _around(E[:2], 8, k)]   # (rejected: the run of a ends early)
    return out


_lines, _expected = {}, {}


def _short(family, n, rng):
    """a member or a near miss of sixteen bytes (the family's letters), for the lines whose '\\n' walks through a 16-byte chunk"""
    return (_pairs(rng, 8) if family in ("exc", "star") else b"b" * 3 + b"a" * 13 if family == "bstar" else b"a" * 16)


def lines(case):
    """The lines of a case (bytes, no '\\n' inside), the same on every call.  For a full-capacity group case the corpus BEGINS with the
    pair that would show a carry leaking from one group into the next at stripe 1024: a line that makes the top position live, and -
    from the next stripe on where the first fits into one, so that neighbouring groups of a wave step them side by side - a line that
    is rejected unless a 1 arrives in its position 0 mid-line."""
    if case.id in _lines:
        return _lines[case.id]
    rng = random.Random(case.id)
    family, n = case.family, case.n
    out_c = _fam(family, n)[3]
    fam = _family_lines(family, n, case.inst, rng)
    short = _short(family, n, rng)
    out = []
    if case.engine == "group" and case.edge == "full" and family != "star":
        top = max((t for t in fam if accepts(case, t)), key=len)
        out.append(top)
        if len(top) + 1 < 1024:
            out.append(short[:1] * (1024 - len(top) - 2))      # the next line begins at byte 1024
        out.append(out_c + min((t for t in fam if accepts(case, t)), key=len))
    body = list(fam)
    body += [out_c + short[:1] * d for d in range(58, 69)]   # dead from the first byte on: the '\n' 59 ... 69 bytes behind it
    body += [out_c + short[:1] * 1100, b"", b""]             # a dead line longer than a stripe of 1024; empty lines
    rng.shuffle(body)
    # sixteen lines in a row of 17 bytes each with the '\n': it sits on every byte of a 16-byte chunk in turn
    body[len(body) // 2:len(body) // 2] = [short, short[:15] + out_c] * 8
    out += body
    out.append(short)                                        # (the last line is not empty: without a final '\n' it would be no line)
    assert all(b"\n" not in t for t in out)
    _lines[case.id] = out
    return out


def corpus(case, final_newline=True):
    return b"\n".join(lines(case)) + (b"\n" if final_newline else b"")


def oracle_is_reference(case):
    return _fam(case.family, case.n)[2] is None


def expected(case):
    """The reference's verdict per line (numpy uint8, read-only): the closed form, or the oracle for the one family without"""
    if case.id not in _expected:
        import numpy as np
        if oracle_is_reference(case):
            from pyoracle import OracleRegex
            o = OracleRegex(case.pattern)
            v = np.array([1 if o.accepts(t) else 0 for t in lines(case)], dtype=np.uint8)
        else:
            v = np.array([1 if accepts(case, t) else 0 for t in lines(case)], dtype=np.uint8)
        v.setflags(write=False)
        _expected[case.id] = v
    return _expected[case.id]


def edge_lines(case, limit=6):
    """indices of a few lines for the facade (one string per call): accepted and rejected, short and the longest, none with a 0x00 (a C
    string ends there)"""
    ls, want = lines(case), expected(case)
    idx = [i for i, t in enumerate(ls) if b"\x00" not in t]
    idx.sort(key=lambda i: (-len(ls[i]), i))
    long_ones = [i for i in idx if want[i]][:2] + [i for i in idx if not want[i]][:2]
    short_ones = [i for i in reversed(idx) if want[i]][:1] + [i for i in reversed(idx) if not want[i] and ls[i]][:1]
    return (long_ones + short_ones)[:limit]


def _case(engine, family, n, inst, edge=""):
    pattern, nbits = pattern_of(family, n), positions(family, n)
    tag = "G%dK%d-m%d%s" % (inst[1], inst[2], inst[3], "s" if inst[4] else "") if engine == "group" else \
          "WL%d-%s" % (inst[1], "front" if inst[2] else "all") if engine == "wave" else "WR%d-%s" % (inst[1], "lds" if inst[2] else "l2")
    return Case("%s-%s-%s-%d%s" % (engine, tag, family, nbits, "-" + edge if edge else ""), engine, family, pattern, n, nbits, inst, edge)


def _n_for(family, nbits, floor=False):
    """the family's parameter for `nbits` positions (exc: the nearest 4k + 2, not above / not below)"""
    if family == "exc":
        return (nbits - 2) // 4 if floor else -(-(nbits - 2) // 4)
    return nbits - {"carry3": 3, "bstar": 2, "chain1": 1, "chainx": 1, "selfhi": 2}[family]


def _table():
    out = []
    build_of = {"carry3": (2, True), "bstar": (2, False), "chain1": (0, False), "selfhi": (0, False), "exc": (0, False), "star": (0, False)}
    low = GROUP_MIN_BITS
    for i, (G, K) in enumerate(GROUP_FORMS):
        cap = 32 * G * K
        for family in ("carry3", "bstar", "chain1", "selfhi", "exc"):
            out.append(_case("group", family, _n_for(family, cap, floor=True), ("group", G, K) + build_of[family], "full"))
        for family in ("carry3", "bstar", "selfhi" if i % 2 else "chain1", "exc"):
            out.append(_case("group", family, _n_for(family, low), ("group", G, K) + build_of[family], "low"))
        low = cap + 1
    out.append(_case("group", "star", (700, 800), ("group", 16, 3, 0, False)))
    out.append(_case("group", "star", (1400, 1600), ("group", 32, 3, 0, False)))
    # ---- wave-resident: the chain at the upper edge W == 64 WL and the lower edge W == 64 WL_prev + 1 of every width the front end
    # admits (a{1,n} up to 21 846 positions, a{n} up to 32 769), FRONT with exceptions, !FRONT by the self term, !FRONT by exceptions
    widths = WAVE_WIDTHS[:-1]
    for i, WL in enumerate(widths):
        cap = 2048 * WL
        if WL <= 16:
            family = "chain1" if WL <= 8 else "chainx"
            out.append(_case("wave", family, _n_for(family, cap), ("wave", WL, True), "full"))
        if i:
            out.append(_case("wave", "chainx", 2048 * widths[i - 1], ("wave", WL, True), "low"))
    for family, WL, nbits in (("carry3", 1, 2048), ("bstar", 2, 4096), ("carry3", 3, 4097), ("bstar", 4, 8192), ("heads", 6, 12288), ("carry3", 8, 16384),
                              ("bstar", 12, 21847), ("heads", 16, 32763)):
        n = (12, nbits - 13) if family == "heads" else _n_for(family, nbits)
        out.append(_case("wave", family, n, ("wave", WL, True)))
    for WL in widths[1:]:
        out.append(_case("wave", "selfhi", _n_for("selfhi", min(2048 * WL, 32769)), ("wave", WL, False)))
    for WL in widths[1:-1]:
        out.append(_case("wave", "exc", min(_n_for("exc", 2048 * WL, floor=True), 7000), ("wave", WL, False)))
    # ---- sparse: rows in LDS at every row count, rows from HBM/L2 where the many-class family reaches, exceptions across blocks
    out.append(_case("sparse", "carry3", _n_for("carry3", 2048), ("sparse", 1, True), "full"))
    out.append(_case("sparse", "bstar", _n_for("bstar", 4096), ("sparse", 2, True), "full"))
    out.append(_case("sparse", "carry3", _n_for("carry3", 4097), ("sparse", 4, True), "low"))
    out.append(_case("sparse", "selfhi", _n_for("selfhi", 16384), ("sparse", 8, True), "full"))
    out.append(_case("sparse", "chainx", _n_for("chainx", 32768), ("sparse", 16, True), "full"))
    out.append(_case("sparse", "exc", 1023, ("sparse", 2, True)))
    out.append(_case("sparse", "exc", 4095, ("sparse", 8, True)))
    out.append(_case("sparse", "heads", (96, 3000), ("sparse", 2, False)))          # 98 classes
    out.append(_case("sparse", "heads", (48, 6000), ("sparse", 4, False)))          # 50 classes
    out.append(_case("sparse", "heads", (24, 9000), ("sparse", 8, False)))          # 26 classes
    out.append(_case("sparse", "heads", (12, 17000), ("sparse", 16, False)))        # 14 classes
    # 32 rows begin at 32 769 positions, the most the front end admits (65 536 reference states, two per position): a{32768}, and seven
    # runs of as many letters - eight classes - for the rows from HBM/L2
    out.append(_case("sparse", "chainx", 32768, ("sparse", 32, True), "low"))
    out.append(_case("sparse", "segs", (4682, 4682, 4681, 4681, 4681, 4681, 4680), ("sparse", 32, False), "low"))
    assert len({c.id for c in out}) == len(out)
    return out


CASES = _table()

# the smallest size of each family that would select WL 32 (49 153 positions): the front end refuses every one
BEYOND_THE_FRONT_END = [pattern_of(f, _n_for(f, 49153)) for f in ("carry3", "bstar", "chain1", "chainx", "selfhi", "exc")] + [pattern_of("heads", (12, 49140))]
