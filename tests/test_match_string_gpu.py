"""rrx_match_string on the device against closed-form references (long_string_cases.py; pinned to the oracle and checked for
strength by test_match_string_lowering.py): pattern families whose chunk maps neither converge nor commute, at the lengths,
table sizes and NFA widths where the chunking, the slots, the batches of step A', the composition levels and the hand-over to
the one-item path change."""
import numpy as np
import pytest
import torch

import long_string_cases as L
import roaringregex_amd as rr

pytestmark = pytest.mark.gpu

TABLE = (rr.ENGINE_AUTO, rr.ENGINE_DFA)
ALL = (rr.ENGINE_AUTO, rr.ENGINE_DFA, rr.ENGINE_NFA)


def run(cases, engines):
    """Every case on every engine; all mismatches reported together.  The set has to hold both verdicts."""
    assert {c.want for c in cases} == {True, False}
    compiled, bad = {}, []
    for c in cases:
        dev = torch.from_numpy(c.data).cuda()
        for e in engines:
            r = compiled.get((c.pattern, e)) or compiled.setdefault((c.pattern, e), rr.RRegex(c.pattern, e))
            got = r.match_string(dev)
            if got != c.want:
                bad.append((c.tag, r.engine_name, "got", got, "want", c.want))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ table path
@pytest.mark.parametrize("family", ["P3", "U"])
def test_table_geometry(family):
    """The 1 KiB threshold; 127, 128, 129 and 1024 chunks of 256 bytes with a last chunk of 0, 1 and 255 bytes over; the chunk
    size changing at 256 KiB; 384 chunks of 1 KiB.  P3 takes the slots (all four in use), U(5) is stepped from every state."""
    run(L.geometry_cases(family), TABLE)


def test_table_three_levels():
    """One string of 1024 * 16384 + 1 bytes: 16385 chunks, the smallest count that needs three levels - and two groups at
    level 2, the one place where a level written over an area still being read would show."""
    c = L.three_level_case()
    dev = torch.from_numpy(c.data).cuda()
    for e in TABLE:
        assert rr.RRegex(c.pattern, e).match_string(dev) == c.want, (c, e)


@pytest.mark.parametrize("k", [5, 7])
def test_table_every_chunk_flagged(k):
    run(L.rotation_cases(k), TABLE)


@pytest.mark.parametrize("k", [5, 7])
def test_table_flagged_and_unflagged_chunks_in_one_batch(k):
    run(L.reset_cases(k), TABLE)


@pytest.mark.parametrize("regime", list(L.K_BLOCK))
def test_table_chunks_per_workgroup(regime):
    """per_block = 256 / D at 3, 2 and 1, the largest admitted table (D = 254), and D = 257: the one-item path, still exact."""
    run(L.per_block_cases(regime), TABLE)


# ------------------------------------------------------------------------------------------------ both paths
def test_bytes_outside_the_domain_reject():
    run(L.domain_cases("P3", None, L.DOMAIN_TABLE_N, 256), TABLE)
    run(L.domain_cases("U", L.GEOMETRY_K, L.DOMAIN_TABLE_N, 256), TABLE)
    run(L.domain_cases("P3", None, L.DOMAIN_NFA_N, 1024), (rr.ENGINE_NFA,))
    run(L.domain_cases("U", L.K_WIDTH[2], L.DOMAIN_NFA_N, 1024), (rr.ENGINE_NFA,))


def test_a_string_at_an_odd_address():
    """rrx.h asks for no alignment of d_bytes: dev[1:], dev[7:] and dev[16:] of one buffer, on the table path (long_walk steps
    bytes where the chunk does not start on a 16-byte boundary) and on the NFA path (long_rows_nfa_kernel now does the same)."""
    _, buf = L.odd_address_buffer()
    dev = torch.from_numpy(buf).cuda()
    assert dev.data_ptr() % 16 == 0
    want = [L.accepts_p3(buf[o:]) for o in L.ODD_OFFSETS]
    assert set(want) == {True, False}
    for e in (rr.ENGINE_DFA, rr.ENGINE_NFA):
        r = rr.RRegex(L.P3, e)
        got = [r.match_string(dev[o:]) for o in L.ODD_OFFSETS]
        assert got == want, (r.engine_name, got, want)


# ------------------------------------------------------------------------------------------------ NFA path
def test_nfa_one_word():
    """32 KiB - 1 stays on one lane; 32, 33 (a last chunk of one byte, and of 1019) and 35 chunks of 1 KiB: 33 is odd at every level."""
    run(L.nfa_cases("P3", None), ALL)


@pytest.mark.parametrize("W", list(L.K_WIDTH))
def test_nfa_width(W):
    """U(k) with 2 ... 8 words per set (5 and 7 run the kernels instantiated at 6 and 8)."""
    run(L.nfa_cases("U", L.K_WIDTH[W]), ALL)


def test_nfa_more_than_256_positions_falls_back_to_one_lane():
    run(L.nfa_cases("U", L.K_NFA_FALLBACK), ALL)
