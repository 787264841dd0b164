#!/usr/bin/env python3
"""Writes tests/golden/table_forms.json: for the known-answer patterns (kat.json: kat and big_states), the fixed patterns of
tests/patterns.py and the patterns tests/test_abi_errors.py names, under every requested table engine and AUTO, what the
library compiles them to: (engine, engine_name, contains_engine_name, contains_states), or null where the compile is refused
(contains_engine_name null: no contains table).  Host only: no GPU is touched.

The file records the behaviour of the build it is generated with, so that a change of the fit rules or of AUTO's order shows
as a diff of the fixture (tests/test_lowering.py: test_table_forms_are_the_recorded_ones).  Regenerate it only on purpose:
    python tests/golden/make_table_forms.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import roaringregex_amd as rr  # noqa: E402
from patterns import EMAIL, K1000, K1000_CONTAINS, KAT, U2  # noqa: E402

ENGINES = ("ENGINE_AUTO", "ENGINE_NFA", "ENGINE_DFA", "ENGINE_DFA_GLOBAL", "ENGINE_DFA2")
ABI_ERRORS = ["abc", "a{1,300}", "(a|b)*a(a|b){40}", "(a|b)*a(a|b){600}"]


def patterns():
    pats = [k["pattern"] for k in KAT["kat"]] + [b["pattern"] for b in KAT["big_states"]] + [EMAIL, U2, K1000, K1000_CONTAINS] + ABI_ERRORS
    return list(dict.fromkeys(pats))


def forms(pattern, engine):
    try:
        r = rr.RRegex(pattern, getattr(rr, engine))
    except rr.RRegexError:
        return None
    try:
        contains = r.contains_engine_name
    except rr.RRegexError:
        contains = None
    return [r.engine, r.engine_name, contains, r.contains_states]


if __name__ == "__main__":
    out = {"engines": list(ENGINES), "forms": [{"pattern": p, "by_engine": [forms(p, e) for e in ENGINES]} for p in patterns()]}
    path = os.path.join(HERE, "table_forms.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path, len(out["forms"]), "patterns")
