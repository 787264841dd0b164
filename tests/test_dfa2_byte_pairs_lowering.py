"""The byte-wide pair table of the stride-2 match table (csrc/device.hpp: Dfa2Device::P8), checked on the host: no GPU needed.
tests/cpp/dfa2_byte_pairs_driver.cpp packs the match image of every known-answer pattern and of the benchmark's patterns the way
the library does and compares P8 with the u16 table entry by entry, as numbered and in a random order; it aborts on a mismatch.
Built as its own program with g++ -fsanitize=address,undefined, like the host-pipeline driver (test_lowering.py)."""
import os
import subprocess

import bench
import roaringregex_amd as rr
from patterns import EMAIL, K1000, K1000_CONTAINS, KAT, U2
from program_replay import host_pipeline_sources


def test_byte_wide_pair_table_equals_the_u16_table(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "roaringregex_amd", "csrc")
    exe = str(tmp_path / "dfa2_byte_pairs_asan")
    # (the translation units are compiled side by side, unoptimised: the driver runs for a second or two, the compiler is the cost)
    flags = ["g++", "-std=c++17", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", "-I", csrc]
    srcs = [os.path.join(root, "tests", "cpp", "dfa2_byte_pairs_driver.cpp")] + host_pipeline_sources()
    objs = [str(tmp_path / (os.path.basename(f) + ".o")) for f in srcs]
    jobs = [subprocess.Popen(flags + ["-c", f, "-o", o]) for f, o in zip(srcs, objs)]
    assert all(j.wait() == 0 for j in jobs)
    subprocess.check_call(flags + objs + ["-o", exe])
    pats = [k["pattern"] for k in KAT["kat"]] + [EMAIL, U2, "a{1,300}", K1000, K1000_CONTAINS] + sorted(bench.patterns().values())
    pats = list(dict.fromkeys(p for p in pats if "\n" not in p))
    out = subprocess.run([exe], input=("\n".join(pats) + "\n").encode("latin-1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stderr.decode("latin-1")[-3000:]
    lines = out.stdout.decode("latin-1").splitlines()
    assert lines[-1].startswith("done %d " % len(pats)), lines[-1]
    seen = {}
    for p, line in zip(pats, lines):
        f = line.split()
        # the driver and the shipped library agree on which patterns have a stride-2 program (rrx_program_words kind 5)
        has = False
        try:
            r = rr.RRegex(p)
            has = r.engine_name == "dfa-stride2-table"
        except rr.RRegexError:
            pass
        assert (f[1] == "stride2") == has, (p[:60], line)
        if has:
            w = r.program(rr.ENGINE_DFA2)
            cols, rep, chosen = int(f[5]), int(f[7]), int(f[9])
            assert (int(w[0]), int(w[1])) == (int(f[3]), cols), (p[:60], line)
            assert chosen == int(((cols - 1) * 4 << rep) <= 255), (p[:60], line)
            seen[p] = (cols, rep, chosen)
    # a table on each side of the bound, among the real patterns
    assert any(c for _, _, c in seen.values()) and any(not c for _, _, c in seen.values()), seen
    # the headline: 46 pair columns, one copy of T2 (its offsets reach 180)
    assert seen[U2] == (46, 0, 1), seen[U2]
    # a small table is replicated; its offsets scale with the copies, and the rule is applied to the scaled ones
    # (a{1,300}: two copies, offsets up to 48 - the byte-wide form; the email regex: 32 copies of a 200-byte table, offsets up
    # to 9 * 4 * 32 = 1152 - it stays on the u16 table)
    assert seen["a{1,300}"] == (7, 1, 1), seen["a{1,300}"]
    assert seen[EMAIL] == (10, 5, 0), seen[EMAIL]
