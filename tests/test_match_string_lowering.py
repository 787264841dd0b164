"""rrx_match_string on the CPU: the references and the strength of the device tests in test_match_string_gpu.py.

* The closed forms of long_string_cases.py equal the oracle on random strings of up to 64 KiB per family - after that the device
  tests may use them where the oracle would take long.
* A chunk-composition model of match_long_dfa / match_long_nfa (chunk maps of the plain table's DfaReplay, composed in groups
  of 128 / pairwise) equals the oracle on the device tests' strings.
* TEST STRENGTH, deterministically: run with one of five mutations - two chunks of a group swapped, a group composed in the
  reverse order, its last chunk dropped, its first chunk taken twice, at level 2 group g + 1 read for group g - the model has
  to change the verdict of at least one string of every device case set whose family has maps that do not commute.  The
  flipped string is named (run with -s to see the table).
* The same check on the five patterns of test_gpu_parity.py::test_one_long_string_is_stepped_in_parallel_chunks records what
  that test misses.
* The regimes the case sets are meant to reach are read from the program dumps and asserted: a change in the lowering that moves
  a pattern out of its regime fails here."""
import functools
import random

import numpy as np
import pytest

import long_string_cases as L
import roaringregex_amd as rr
from patterns import U2
from program_replay import DfaReplay
from pyoracle import OracleRegex


@functools.lru_cache(maxsize=None)
def dfa_of(pattern):
    return DfaReplay(rr.RRegex(pattern, rr.ENGINE_DFA).program(rr.ENGINE_DFA))


@functools.lru_cache(maxsize=None)
def oracle_of(pattern):
    return OracleRegex(pattern)


def nfa_shape(pattern):
    w = rr.RRegex(pattern, rr.ENGINE_NFA).program(rr.ENGINE_NFA)
    return int(w[0]), int(w[1])                       # W, nbits


# ------------------------------------------------------------------------------------------------ closed forms
def _random_strings(family, k, rng):
    """A few hundred strings: most short, some up to 64 KiB; in the domain, at its edge (a multiple of k, one more) and outside."""
    out = []
    sizes = [rng.randrange(0, 120) for _ in range(260)] + [rng.randrange(1000, 65537) for _ in range(40)]
    for i, n in enumerate(sizes):
        if family in ("Z", "U") and i % 3 == 0:
            n -= n % k                                # Z(k) accepts
        t = bytearray(rng.choice(b"ab") for _ in range(n))
        if family == "U":
            t = bytearray(b"c") + t
        if family == "R":
            t = bytearray()
            while len(t) < n:                         # segments of whole multiples of k, now and then one off
                m = k * rng.randrange(0, 1 + max(1, n // (4 * k))) + (1 if rng.random() < 0.05 else 0)
                t += bytearray(rng.choice(b"ab") for _ in range(m)) + b"c"
            if rng.random() < 0.5:
                t = t[:-1]
        if t and i % 11 == 0:
            t[rng.randrange(len(t))] = rng.choice(b"c\x00\xc3dA")      # a foreign byte somewhere
        if family == "U" and i % 17 == 0:
            t = t[1:]                                 # no `c` in front
        out.append(bytes(t))
    return out


@pytest.mark.parametrize("family,k", [("P3", None), ("Z", 5), ("Z", 7), ("U", 5), ("U", 27), ("U", 84), ("U", 85), ("U", 250), ("R", 5), ("R", 7)])
def test_closed_form_equals_the_oracle(family, k):
    pattern, fn = L.reference(family, k)
    o = oracle_of(pattern)
    seen = set()
    for s in _random_strings(family, k, random.Random(1000 + (k or 0))):
        want = o.accepts(s)
        assert fn(s) == want, (family, k, len(s), s[:60])
        seen.add(want)
    assert seen == {True, False}


def test_the_starred_alternative_falls_through():
    """Why U(k) carries a `c`: the reference's `x*|y*` is x*y*, so P3|Z(k) is not the union of the two."""
    assert oracle_of("x*|y*").accepts("xxyy")
    o = oracle_of(L.P3 + "|" + L.Z(5))
    assert o.accepts("a" * 8) and not L.accepts_p3(b"a" * 8) and 8 % 5          # aaa from P3, then aaaaa from Z(5)
    assert not oracle_of(L.U(5)).accepts("c" + "a" * 8)


# ------------------------------------------------------------------------------------------------ regimes, read from the dumps
def test_table_regimes():
    assert dfa_of(L.P3).nstates == L.K_LONG_SLOTS == 4                         # 3 live states and the dead row
    assert dfa_of(L.Z(5)).nstates == 6 and dfa_of(L.Z(7)).nstates == 8         # more than the slots
    assert dfa_of(L.R(5)).nstates == 6 and dfa_of(L.R(7)).nstates == 8
    D = {name: dfa_of(L.U(k)).nstates for name, k in L.K_BLOCK.items()}
    assert D == {"D<=85": 83, "D 86..128": 128, "D 129..253": 131, "D=254": 254, "D>=255": 257}, D
    assert 256 // D["D<=85"] == 3 and 256 // D["D 86..128"] == 2 and 256 // D["D 129..253"] == 1 and 256 // D["D=254"] == 1
    assert D["D=254"] == L.K_LONG_MAX_STATES < D["D>=255"]
    assert dfa_of(L.U(L.GEOMETRY_K)).nstates == 17
    for p in (L.P3, L.Z(5), L.R(7)) + tuple(L.U(k) for k in L.K_BLOCK.values()):
        assert rr.RRegex(p).engine == rr.ENGINE_DFA                            # AUTO stays on a table: the long path is taken


def test_nfa_regimes():
    assert nfa_shape(L.P3) == (1, 7)
    instantiated = {1: 1, 2: 2, 3: 3, 4: 4, 5: 6, 6: 6, 7: 8, 8: 8}            # RRX_NFA_DISPATCH
    for W, k in L.K_WIDTH.items():
        w, nbits = nfa_shape(L.U(k))
        assert (w, nbits) == (W, k + 9) and nbits <= L.NFA_MAX_BITS, (k, w, nbits)
    assert {instantiated[W] for W in L.K_WIDTH} | {1} == {1, 2, 3, 4, 6, 8}
    w, nbits = nfa_shape(L.U(L.K_NFA_FALLBACK))
    assert nbits == 259 > L.NFA_MAX_BITS


def test_slot_regimes():
    """What step B meets: P3 exactly four distinct prefix states in every chunk (all slots in use), Z(k) k + 1 (every chunk
    flagged), R(k) 2 or k + 1 - and both kinds inside one batch of 256 / D chunks of step A'."""
    for c in L.geometry_cases("P3"):
        n = c.data.size
        if n >= L.TABLE_FROM and n <= 256 * 130:
            full = n // L.long_chunk(n)
            assert (L.prefix_distinct(dfa_of(L.P3), c.data, L.long_chunk(n))[:full] == 4).all(), c
    for k in (5, 7):
        d = dfa_of(L.Z(k))
        for c in L.rotation_cases(k):
            full = c.data.size // 256
            assert (L.prefix_distinct(d, c.data, 256)[:full] == k + 1).all(), c
        d = dfa_of(L.R(k))
        per_block = 256 // d.nstates
        for c in L.reset_cases(k):
            cnt = L.prefix_distinct(d, c.data, 256)
            assert set(cnt[:-1]) == {2, k + 1}, (c, set(cnt))
            flagged = cnt > L.K_LONG_SLOTS
            mixed = [b for b in range(0, len(cnt), per_block) if flagged[b:b + per_block].any() and not flagged[b:b + per_block].all()]
            assert len(mixed) == (len(cnt) + per_block - 1) // per_block, (c, "every batch holds both kinds")


# ------------------------------------------------------------------------------------------------ model and mutations
def _case_sets():
    """name -> (cases, group of the composition, chunk size of a length, mutations that must flip a string of the set)"""
    table = lambda n: L.long_chunk(n)
    first4 = L.MUTATIONS[:4]
    sets = {
        "geometry P3": (L.geometry_cases("P3") + [L.three_level_case()], 128, table, L.MUTATIONS),
        "geometry U(%d)" % L.GEOMETRY_K: (L.geometry_cases("U"), 128, table, first4),
        "odd address P3, table": ([L.Case("odd address +%d" % o, "P3", None, L.odd_address_buffer()[1][o:]) for o in L.ODD_OFFSETS], 128, table, ()),
        "domain P3, table": (L.domain_cases("P3", None, L.DOMAIN_TABLE_N, 256), 128, table, ()),
        "domain U, table": (L.domain_cases("U", L.GEOMETRY_K, L.DOMAIN_TABLE_N, 256), 128, table, ()),
        "nfa P3": (L.nfa_cases("P3", None), 2, lambda n: 1024, L.MUTATIONS),
    }
    for name, k in L.K_BLOCK.items():
        # (D >= 255: one lane steps the string, nothing is composed - the model is run all the same, no mutation applies)
        sets["per_block %s U(%d)" % (name, k)] = (L.per_block_cases(name), 128, table, first4 if name != "D>=255" else ())
    for W, k in L.K_WIDTH.items():
        sets["nfa W=%d U(%d)" % (W, k)] = (L.nfa_cases("U", k), 2, lambda n: 1024, L.MUTATIONS)
    for k in (5, 7):
        sets["rotation Z(%d)" % k] = (L.rotation_cases(k), 128, table, ("drop_last", "first_twice"))   # rotations commute
        sets["reset R(%d)" % k] = (L.reset_cases(k), 128, table, ())
    return sets


CASE_SETS = _case_sets()


INNER = " (inner groups)"          # the same mutation with the last group of every level - the end of the string - left intact


def _mutation_table(cases, group, chunk_of, oracle_limit=1 << 20):
    """Faithful model == the case's reference (== the oracle up to 1 MiB); -> {mutation: tag of the first string it flips}."""
    flips = {}
    for c in cases:
        n = c.data.size
        if n < (L.TABLE_FROM if group == 128 else L.NFA_FROM):
            continue                                                    # one lane: nothing is composed
        d = dfa_of(c.pattern)
        maps = L.chunk_maps(d, c.data, chunk_of(n))
        assert L.model_verdict(d, maps, group) == c.want, (c, "faithful model")
        if n <= oracle_limit:
            assert oracle_of(c.pattern).accepts(c.data.tobytes()) == c.want, (c, "oracle")
        for m in L.MUTATIONS:
            for inner in (False, True):
                key = m + (INNER if inner else "")
                if key not in flips and L.model_verdict(d, maps, group, m, spare_last=inner) != c.want:
                    flips[key] = c.tag
    return flips


@pytest.mark.parametrize("name", sorted(CASE_SETS))
def test_device_case_set_against_model_oracle_and_mutations(name):
    cases, group, chunk_of, required = CASE_SETS[name]
    assert {c.want for c in cases} == {True, False}, name
    flips = _mutation_table(cases, group, chunk_of)
    for m in [m + i for m in L.MUTATIONS for i in ("", INNER)]:
        print("%-28s %-30s %s" % (name, m, flips.get(m, "-")))
    missing = [m + i for m in required for i in ("", INNER) if m + i not in flips]
    assert not missing, (name, "no string of the set notices", missing)


def test_nfa_fallback_set_has_both_verdicts():
    cases = L.nfa_cases("U", L.K_NFA_FALLBACK)
    assert {c.want for c in cases} == {True, False}
    for c in cases:
        assert oracle_of(c.pattern).accepts(c.data.tobytes()) == c.want, c


# ------------------------------------------------------------------------------------------------ the old test's patterns
def _old_cases():
    """The strings of test_gpu_parity.py::test_one_long_string_is_stepped_in_parallel_chunks, built the same way."""
    rng = np.random.default_rng(21)
    abc = np.frombuffer(b"ab", dtype=np.uint8)
    cases = []
    for n in (1023, 1024, 1025, 2047, 2048, 2049, 3000, 8191, 32 * 1024 - 1, 32 * 1024, 32 * 1024 + 1, 100_003, 262143, 262145, (1 << 20) + 17,
              5 * (1 << 20) + 1023, 20 * (1 << 20) + 5):
        body = abc[rng.integers(0, 2, size=n)]
        for tail in (b"abb", b"aba"):
            t = body.copy()
            t[-3:] = np.frombuffer(tail, dtype=np.uint8)
            cases.append(("(a|b)*abb", t))
    text = np.frombuffer(b"the quick brown fox\n", dtype=np.uint8)
    big = np.tile(text, 60000)
    hit = big.copy(); hit[777_777:777_780] = np.frombuffer(b"abc", dtype=np.uint8)
    cases += [(".*abc.*", big), (".*abc.*", hit), ("abc", hit), ("(the quick brown fox.)*", big), ("(the quick brown fox.)*", big[:-1])]
    high = hit.copy(); high[999_999] = 0xC3
    cases.append((".*abc.*", high))
    url = np.frombuffer(b"https://www.example.com/" + b"a/b-c_d.e" * 30000 + b"?q=1", dtype=np.uint8)
    cases += [(U2, url), (U2, url[:-4]), (U2, np.concatenate([url, np.frombuffer(b" x", dtype=np.uint8)]))]
    runs = np.frombuffer((b"a" * 37 + b"b") * 2500, dtype=np.uint8)
    broken = runs.copy(); broken[50_000:50_120] = ord("a")
    cases += [("(a{1,100}b)*", runs), ("(a{1,100}b)*", broken), ("(a{1,100}b)*", runs[:-1])]
    return cases


# Which mutations of the table path's composition (groups of 128) flip at least one string of the old test, per pattern, as the
# model shows it; "(inner groups)" = the same mutation with the last group of every level left intact.  This DISAGREES in part
# with the reading that led to these files (which expected the old test to notice nothing but a dropped chunk, through `fox`):
#   * `.*abc.*` and `abc` notice nothing, as read: one hit or one miss decides.
#   * `(a|b)*abb` is definite, but its strings of 128 * 256 + 1 and 1024 * 256 + 1 bytes end in a chunk of ONE byte, so the three
#     bytes that decide span the last chunk of an inner group: a reversed group or a dropped last chunk shows there.
#   * the live maps of `fox` are PARTIAL rotations (a chunk that starts at phase f is dead from every other state), and those do
#     not commute: every mutation of one level shows.
#   * U2 and a{1,100} notice a few, through their last groups mostly.
#   * NO old pattern notices `next_group`: the one string with two groups at level 2 is the definite automaton's.
_I = " (inner groups)"
OLD_PATTERNS_NOTICE = {
    "(a|b)*abb": {"drop_last", "drop_last" + _I, "reverse_order", "reverse_order" + _I, "swap_chunks"},
    ".*abc.*": set(),
    "abc": set(),
    "(the quick brown fox.)*": {m + i for m in ("swap_chunks", "reverse_order", "drop_last", "first_twice") for i in ("", _I)},
    "U2": {"drop_last", "first_twice", "first_twice" + _I, "reverse_order", "reverse_order" + _I},
    "(a{1,100}b)*": {"drop_last", "reverse_order"},
}


def test_what_the_old_patterns_notice():
    got = {}
    for pattern, t in _old_cases():
        name = "U2" if pattern == U2 else pattern
        d = dfa_of(pattern)
        assert d.nstates <= L.K_LONG_MAX_STATES
        maps = L.chunk_maps(d, t, L.long_chunk(t.size))
        want = L.model_verdict(d, maps)
        got.setdefault(name, set()).update(m + (INNER if inner else "") for m in L.MUTATIONS for inner in (False, True)
                                           if L.model_verdict(d, maps, 128, m, spare_last=inner) != want)
    for name in got:
        print("%-26s notices: %s" % (name, ", ".join(sorted(got[name])) or "nothing"))
    assert got == OLD_PATTERNS_NOTICE
