"""Pattern sets (rrx_multi) on the CPU: the groups' product tables (rrx_multi_program_words) replayed item by item, the groups'
masks ORed, against the brute force over every item's substrings for every member - and the shape of the grouping itself."""
import ctypes as C
import time

import numpy as np
import pytest

import roaringregex_amd as rr
from contains_cases import EXPLODING
from multi_cases import SETS, MultiReplay, items_of, replay, want_column, want_masks

ROW_LIMITS = (8, 16)


@pytest.mark.parametrize("name", list(SETS))
def test_every_bit_against_the_brute_force(name):
    items, want = items_of(name), want_masks(name)
    m = rr.RMulti(SETS[name])
    assert len(m) == len(SETS[name])
    got = replay(m, items)
    assert got.shape == want.shape                      # (no item is left out)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (name, int(bad[0]), items[bad[0]], hex(int(got[bad[0]])), hex(int(want[bad[0]])))
    k = len(SETS[name])
    for j in range(k):                                  # the oracle alone: every member that can show both verdicts does
        col = (want >> np.uint32(j)) & 1
        if rr.RRegex(SETS[name][j]).accepts_empty:
            assert col.all(), (name, j)
        else:
            assert 0 < int(col.sum()) < len(col), (name, j, int(col.sum()))
    assert not (got >> np.uint32(k)).any() if k < 32 else True


@pytest.mark.parametrize("name", list(SETS))
@pytest.mark.parametrize("max_rows", ROW_LIMITS)
def test_row_limits_cut_the_set_into_groups_with_the_same_answers(name, max_rows):
    pats, items = SETS[name], items_of(name)
    one = rr.RMulti(pats)
    cut = rr.RMulti(pats, max_rows=max_rows)
    ngroups = rr._L.rrx_multi_groups(cut._h)
    assert ngroups == cut.groups
    if len(pats) == 1:
        assert ngroups == 1                             # (one member is one group whatever the limit)
    else:
        assert ngroups >= 2, (name, max_rows, ngroups)
    # the group masks partition the set, in set order
    seen = 0
    for g in range(ngroups):
        gm = cut.group_mask(g)
        assert gm and not (gm & seen), (name, g, hex(gm), hex(seen))
        assert gm > seen, "groups are cut in set order"
        seen |= gm
        members = bin(gm).count("1")
        assert cut.group_states(g) <= max_rows or members == 1, (name, g, cut.group_states(g), members)
        assert cut.group_states(g) == MultiReplay(cut.program(g)).nstates
    assert seen == (1 << len(pats)) - 1
    assert cut.group_mask(ngroups) == 0 and cut.group_states(ngroups) == 0 and cut.program(ngroups) is None
    assert (replay(cut, items) == replay(one, items)).all()


@pytest.mark.parametrize("name", list(SETS))
def test_first_hit_and_full(name):
    for max_rows in (0,) + ROW_LIMITS:
        m = rr.RMulti(SETS[name], max_rows=max_rows)
        for g in range(m.groups):
            t = MultiReplay(m.program(g))
            assert (t.mask[:t.first_hit] == 0).all() and (t.mask[t.first_hit:] != 0).all(), (name, max_rows, g)
            assert t.full == int(np.bitwise_or.reduce(t.mask)), (name, max_rows, g)
            assert t.full & ~m.group_mask(g) == 0       # a table sets no bit of another group's members
            assert t.start < t.nstates and (t.next < t.nstates).all() and (t.cls < t.ncls).all()


def test_the_global_build_has_the_same_answers_and_no_lds_limit():
    items = items_of("twelve")
    a, b = rr.RMulti(SETS["twelve"]), rr.RMulti(SETS["twelve"], engine=rr.ENGINE_DFA_GLOBAL)
    assert (replay(a, items) == replay(b, items)).all()
    assert b.groups <= a.groups


def test_empty_languages_and_nullable_members():
    items = items_of("one")[:80]
    m = rr.RMulti(["[]", "a*", "[]", "ab+c"])
    got = replay(m, items)
    assert not (got & 0b0101).any() and ((got & 0b0010) != 0).all()
    assert (((got >> 3) & 1) == want_column("ab+c", "fixed")[:80]).all()
    nothing = rr.RMulti(["[]", "[]"])
    assert nothing.groups == 1 and MultiReplay(nothing.program(0)).full == 0
    assert not replay(nothing, items).any()


def test_a_member_that_does_not_determinise_is_refused_by_its_index():
    with pytest.raises(rr.RRegexError, match=r"pattern 2: .*does not determinise"):
        rr.RMulti(["ab+c", "a*", EXPLODING, "c.*"])
    with pytest.raises(rr.RRegexError, match=r"pattern 1: "):
        rr.RMulti(["ab+c", "(", "c.*"])
    h = C.c_void_p()
    arr = (C.c_char_p * 3)(b"ab+c", EXPLODING.encode(), b"(")
    assert rr._L.rrx_multi_compile(C.cast(arr, C.c_void_p), 2, C.byref(h)) == 4 and not h.value       # RRX_ERR_UNSUPPORTED
    assert b"pattern 1" in rr._L.rrx_last_error()
    arr = (C.c_char_p * 2)(b"ab+c", b"(")
    assert rr._L.rrx_multi_compile(C.cast(arr, C.c_void_p), 2, C.byref(h)) == 1 and not h.value       # RRX_ERR_PATTERN
    assert b"pattern 1" in rr._L.rrx_last_error()


def test_argument_errors():
    h = C.c_void_p()
    one = (C.c_char_p * 1)(b"a")
    many = (C.c_char_p * 33)(*[b"a"] * 33)
    err_arg = 2
    assert rr._L.rrx_multi_compile(C.cast(one, C.c_void_p), 0, C.byref(h)) == err_arg
    assert rr._L.rrx_multi_compile(C.cast(many, C.c_void_p), 33, C.byref(h)) == err_arg
    assert rr._L.rrx_multi_compile(C.cast(many, C.c_void_p), 32, C.byref(h)) == 0 and h.value
    assert rr._L.rrx_multi_patterns(h) == 32
    rr._L.rrx_multi_free(h)
    h = C.c_void_p()
    assert rr._L.rrx_multi_compile(None, 1, C.byref(h)) == err_arg
    assert rr._L.rrx_multi_compile(C.cast(one, C.c_void_p), 1, None) == err_arg
    hole = (C.c_char_p * 2)(b"a", None)
    assert rr._L.rrx_multi_compile(C.cast(hole, C.c_void_p), 2, C.byref(h)) == err_arg and b"pattern 1" in rr._L.rrx_last_error()
    assert rr._L.rrx_multi_compile_ex(C.cast(one, C.c_void_p), 1, rr.ENGINE_NFA, 0, C.byref(h)) == err_arg
    with pytest.raises(rr.RRegexError):
        rr.RMulti([])
    with pytest.raises(rr.RRegexError):
        rr.RMulti(["a"] * 33)
    # the entries refuse null arguments before any device call (this box may have no device at all)
    m = rr.RMulti(["a", "b"])
    buf = (C.c_uint64 * 40)()
    p = C.cast(buf, C.c_void_p)
    assert rr._L.rrx_multi_contains_extents(None, 0, p, p, 1, 0, p, None) == err_arg
    assert rr._L.rrx_multi_contains_extents(m._h, 0, p, None, 1, 0, p, None) == err_arg
    assert rr._L.rrx_multi_contains_extents(m._h, 0, p, p, 1, 0, None, None) == err_arg
    assert rr._L.rrx_multi_contains_items(m._h, None, p, None) == err_arg
    assert rr._L.rrx_multi_contains_extents(m._h, 0, None, None, 0, 0, None, None) == 0        # an empty batch: nothing to do
    assert rr._L.rrx_multi_counts(0, p, 1, None, None) == err_arg
    assert rr._L.rrx_multi_counts(0, None, 1, p, None) == err_arg
    assert rr._L.rrx_multi_plane(0, None, 1, 0, p, None) == err_arg
    assert rr._L.rrx_multi_plane(0, p, 1, 0, None, None) == err_arg
    assert rr._L.rrx_multi_plane(0, p, 1, 32, p, None) == err_arg
    assert rr._L.rrx_multi_groups(None) == 0 and rr._L.rrx_multi_patterns(None) == 0 and rr._L.rrx_multi_program_words(None, 0, None, 0) == 0


def test_a_full_set_compiles_within_the_bound_of_an_oversized_automaton():
    """test_abi_errors.test_oversized_automata_are_refused_quickly gives a refusal 20 seconds; 32 members get no more."""
    t0 = time.time()
    m = rr.RMulti(SETS["thirtytwo"])
    assert time.time() - t0 < 20
    assert len(m) == 32 and m.groups >= 2
