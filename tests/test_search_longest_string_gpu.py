"""rrx_search_longest_string / rrx_contains_string on the device against the closed forms of long_search_cases.py (pinned to the
sequential replay, the brute force and a model of the chunked procedure by test_search_longest_string_lowering.py, which also shows
for every defect of that procedure a case here that it gets wrong).  Every case of at most 1 MiB is also compared with
rrx_search_longest_extents on the one-item batch over the SAME device bytes: the entries' one rule, tested as stated.  (A string
beyond 0xFFFFFFFE bytes is not tested - no test allocates 4 GiB; the refusal on the one-item path is a comparison in strings.cpp.)"""
import numpy as np
import pytest
import torch

import long_search_cases as S
import roaringregex_amd as rr

pytestmark = pytest.mark.gpu

ENGINES = (rr.ENGINE_AUTO, rr.ENGINE_DFA)
ONE_RULE_MAX = 1 << 20


def on_device(c):
    """The case's bytes at an address = c.skew mod 16."""
    buf = torch.empty(c.data.size + c.skew + 16, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    dev = buf[c.skew:c.skew + c.data.size]
    dev.copy_(torch.from_numpy(c.data))
    return dev


def run(cases, nullable=False):
    """Every case on both engines; all mismatches reported together.  The set has to hold both verdicts of contains_string."""
    assert nullable or {c.want == S.NONE for c in cases} == {True, False}
    compiled, bad = {}, []
    for c in cases:
        dev = on_device(c)
        off = torch.tensor([0, c.data.size], dtype=torch.int64, device="cuda")
        for e in ENGINES:
            r = compiled.get((c.pattern, e)) or compiled.setdefault((c.pattern, e), rr.RRegex(c.pattern, e))
            got = r.search_longest_string(dev)
            if got != c.want:
                bad.append((c.tag, r.engine_name, "got", got, "want", c.want))
            found = r.contains_string(dev)
            if found != (c.want != S.NONE):
                bad.append((c.tag, r.engine_name, "contains", found))
            if c.data.size <= ONE_RULE_MAX:
                s, t = r.search_longest_extents(dev, off)
                item = (int(s.item()), int(t.item()))
                if got != item:
                    bad.append((c.tag, r.engine_name, "got", got, "the one-item batch", item))
    assert not bad, bad[:12]


@pytest.mark.parametrize("name", [n for n in S.SET_NAMES if n != "nullable"])
def test_case_set(name):
    """number / W(5) / W(7) positions: starts and ends at 0, at the string's end and around the chunk, group and window edges of
    each pass, matches of 1, 2 and 130 chunks; geometry: every length at which the chunking changes and the hand-over threshold;
    slots and rotation; leftmost beats longer; the one-item path of a{1,300}; the URL tables; odd addresses; NUL and bytes >= 0x80."""
    run(S.small_case_sets()[name])


def test_nullable_patterns():
    """a* and x?y?z?: no backward pass, start 0, the longest accepted prefix - across the first windows' hand-overs and to the end."""
    run(S.small_case_sets()["nullable"], nullable=True)


@pytest.mark.parametrize("which", ["backward", "forward"])
def test_three_levels(which):
    """backward: 1024 * 16384 + 1 bytes, a W(5) match from the first byte to 64 bytes before the end - the backward pass takes 16385
    chunks through three levels in a live state (the forward pass has six windows of two levels at most).  forward: 32 MiB + 69
    bytes, the match from byte 0 into the last chunk of the sixth forward window, which has 16385 chunks - three levels, entered in
    the state the fifth window left.  Each with its variant whose run is one byte longer: the answer is the small match planted
    behind it."""
    for c in (S.three_level_cases() if which == "backward" else S.forward_three_level_cases()):
        dev = on_device(c)
        for e in ENGINES:
            r = rr.RRegex(c.pattern, e)
            assert r.search_longest_string(dev) == c.want, (c, e)
            assert r.contains_string(dev)


def test_short_and_empty_strings():
    """Below the threshold everything is one item: the empty string gives [0, 0) for a nullable pattern and none otherwise."""
    empty = torch.empty(0, dtype=torch.uint8, device="cuda")
    assert rr.RRegex("a*").search_longest_string(empty) == (0, 0) and rr.RRegex("a*").contains_string(empty)
    assert rr.RRegex("ab").search_longest_string(empty) == S.NONE and not rr.RRegex("ab").contains_string(empty)
    dev = torch.from_numpy(np.frombuffer(b"zzabcdz", dtype=np.uint8).copy()).cuda()
    assert rr.RRegex("abcd|c").search_longest_string(dev) == (2, 6)


def test_dfa_global_goes_through_the_one_item_path():
    c = S.small_case_sets()["slots and rotation"][0]
    assert rr.RRegex(c.pattern, rr.ENGINE_DFA_GLOBAL).search_longest_string(on_device(c)) == c.want
