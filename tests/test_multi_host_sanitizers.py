"""The host side of a pattern set - product, minimisation, grouping and pack_multi - under AddressSanitizer + UBSan, over the sets
of multi_cases at several row limits, in the LDS and the global form.  CPU only; the driver is tools/sanitize/multi_product_asan.cpp
(it checks every plan against the members' own tables and aborts on a mismatch)."""
import os
import shutil
import subprocess

import pytest

from multi_cases import SETS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_multi_product_is_clean_under_asan_and_ubsan(tmp_path):
    sets = tmp_path / "sets.txt"
    sets.write_text("".join(" ".join(p.encode("latin-1").hex() for p in pats) + "\n" for pats in SETS.values()))
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "tools", "sanitize"), "multi", "SETS=%s" % sets], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "multi product host pipeline: %d sets, %d plans ok" % (len(SETS), 10 * len(SETS)) in out.stdout, out.stdout[-2000:]
    assert "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-2000:]
