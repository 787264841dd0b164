"""Writes tests/golden/nfa_width_vectors.json: the oracle's verdict for every line of every case of tests/nfa_width_cases.py, one bit
per line (little-endian within a byte, hex), with the line count and the SHA-1 of the corpus the verdicts belong to.  Takes minutes:
the oracle walks the n * n / 2 edges of a{1,n} and (a?){n} byte by byte.  Run it again whenever the case table changes."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(HERE, ".."), os.path.join(HERE, "..", "..", "oracle")):
    sys.path.insert(0, p)
import nfa_width_cases as T  # noqa: E402

out = {}
for case in T.CASES:
    v = T.oracle_vector(case)
    out[case.id] = {"sha1": T.digest(case), "lines": int(len(v)), "accepted": int(v.sum()), "bits": np.packbits(v, bitorder="little").tobytes().hex()}
    print(case.id, len(v), int(v.sum()), flush=True)
with open(T.GOLDEN, "w") as f:
    json.dump(out, f, indent=0, sort_keys=True)
    f.write("\n")
