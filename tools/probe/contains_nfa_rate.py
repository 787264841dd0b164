"""Contains on the NFA lane engine (RRX_OPT_CONTAINS_NFA) against its yardstick, rrx_match_corpus of the same regex on the NFA lane
engine: the same step without the AND-OR per word that gathers S & FIN, so it cannot be slower.  (a|b)*a(a|b){40} and
(a|b)*a(a|b){14} on 1 GiB of a/b lines, EMAIL on the 1 GiB e-mail corpus - for EMAIL also the table path (option 0) -, and the
items form on an offsets array over the same lines (trim 1: the '\\n' is the separator).  One process per config; the variants of
a config alternate launch by launch, device events around every launch, medians of `--launches` launches after warm-up.

The match side is this tree's: the LineNfaEngine kernels compile to the parent commit's instructions
(profiles/contains_nfa_isa_check.txt).

    python tools/probe/contains_nfa_rate.py [--launches 15] [--scale 1.0] [--out profiles/contains_nfa_rate.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CONFIGS = (("ablines", "(a|b)*a(a|b){40}", 1, 1 << 30), ("ablines", "(a|b)*a(a|b){14}", 1, 1 << 30), ("email", "EMAIL", 2, 1 << 30))


def child(kind, pattern, mode, nbytes, launches):
    for p in (ROOT, os.path.join(ROOT, "tools")):
        sys.path.insert(0, p)
    import torch
    from bench import patterns
    import roaringregex_amd as rr
    import synth
    pattern = patterns().get(pattern, pattern)
    host = synth.corpus(kind, 1, nbytes, threads=min(len(os.sched_getaffinity(0)), 16))
    dev = torch.from_numpy(host).cuda()
    c = rr.Corpus(dev)
    ends = torch.nonzero(dev == 10).flatten() + 1
    off = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), ends])
    if int(off[-1]) != dev.numel():
        off = torch.cat([off, torch.tensor([dev.numel()], dtype=torch.int64, device="cuda")])
    nitems = off.numel() - 1
    nfa = rr.RRegex(pattern)
    nfa.set_contains_nfa(mode)
    assert nfa.contains_engine_name == "nfa-shift-and"
    match = rr.RRegex(pattern, rr.ENGINE_NFA)
    match.set_sampled_table(False)
    bits, mbits = nfa.contains_corpus_bits(c), match.match_corpus_bits(c)
    ibits = nfa.contains_extents_bits(dev, off, trim=1)
    calls = {"contains_nfa": lambda: nfa.contains_corpus_bits(c, out=bits), "match_nfa": lambda: match.match_corpus_bits(c, out=mbits),
             "contains_nfa_items": lambda: nfa.contains_extents_bits(dev, off, trim=1, out=ibits)}
    info = {"contains_nfa": {"contained": rr.bitmap_count(bits, c.num_lines)}, "match_nfa": {"accepted": rr.bitmap_count(mbits, c.num_lines)},
            "contains_nfa_items": {"contained": rr.bitmap_count(ibits, nitems), "items": nitems}}
    if mode == 2:                                          # a table exists: the default route beside it
        table = rr.RRegex(pattern)
        tbits = table.contains_corpus_bits(c)
        calls["contains_table"] = lambda: table.contains_corpus_bits(c, out=tbits)
        info["contains_table"] = {"engine": table.contains_engine_name, "contained": rr.bitmap_count(tbits, c.num_lines)}
        assert torch.equal(tbits, bits)
    for _ in range(4):
        for call in calls.values():
            call()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(launches):
        for k, call in calls.items():                      # A, B, ... A, B, ...
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); call(); b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    out = {"config": kind, "pattern": pattern, "bytes": nbytes, "lines": c.num_lines, "words_per_set": match.words_per_set, "launches": launches}
    for k, v in ms.items():
        v.sort()
        med = statistics.median(v)
        out[k] = dict(info[k], ms=round(med, 4), min_ms=round(v[0], 4), max_ms=round(v[-1], 4), **{"TB/s": round(nbytes / med / 1e9, 3)})
    out["contains_over_match"] = round(out["contains_nfa"]["ms"] / out["match_nfa"]["ms"], 3)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=15)
    ap.add_argument("--scale", type=float, default=1.0, help="corpus sizes times this (a quick run)")
    ap.add_argument("--out", default=None, help="append the result lines to this file as well")
    ap.add_argument("--child", nargs=4, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        kind, pattern, mode, nbytes = a.child
        return child(kind, pattern, int(mode), int(nbytes), a.launches)
    for kind, pattern, mode, nbytes in CONFIGS:
        n = int(nbytes * a.scale) // 4096 * 4096
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--launches", str(a.launches), "--child", kind, pattern, str(mode), str(n)],
                           stdout=subprocess.PIPE, text=True, timeout=400)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode:                                   # a fault or a time limit: nothing more is started on the device
            raise SystemExit("child failed with %d: %s %s" % (r.returncode, kind, pattern))
        if a.out:
            with open(a.out, "a") as f:
                f.write(r.stdout)


if __name__ == "__main__":
    main()
