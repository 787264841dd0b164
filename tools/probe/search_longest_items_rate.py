"""rrx_search_longest_extents (leftmost-longest, a lane per item) beside the parent commit's rrx_search_extents (smallest end first)
on the same items: the URL, email and keyword-log texts of bench.py, 1 GiB each, viewed as items (offsets = the line starts, trim 1:
the '\\n' is the separator).

  search_longest   this tree: rrx_search_longest_extents on the batch;
  search_items     the parent commit: rrx_search_extents on the same batch.

WHAT TO EXPECT: the new call reads every item to its end (the starts table has no dead row: no early exit) and then the match once
more; the old call stops at the first byte after which a match ends.  On text where most items match early the new call is slower,
and that is the price of the semantics - the table printed here says how much, it is not a regression to chase.

The parent's side runs from a second checkout under .oldtree/ (git archive <commit> | tar -x -C .oldtree; build there), alternating
with this tree's, a fresh process each; device events around every launch, median and spread of `--launches` launches (at least
twelve) after warm-up.

    python tools/probe/search_longest_items_rate.py [--old .oldtree] [--launches 15] [--scale 1.0]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CONFIGS = (("url", "U2", 1 << 30), ("email", "EMAIL", 1 << 30), ("kwlog", "K1000C", 1 << 30))


def child(tree, side, kind, pkey, nbytes, launches):
    for p in (tree, os.path.join(tree, "tools")):
        sys.path.insert(0, p)
    sys.path.insert(0, ROOT)                   # bench.patterns() only (the same in both trees)
    import numpy as np
    import torch
    from bench import patterns
    sys.path.remove(ROOT)
    import roaringregex_amd as rr
    import synth
    assert os.path.dirname(os.path.abspath(rr.__file__)).startswith(os.path.abspath(tree)), rr.__file__
    r = rr.RRegex(patterns()[pkey])
    host = synth.corpus(kind, 1, nbytes, threads=min(len(os.sched_getaffinity(0)), 16))
    host = host[:int(np.nonzero(host == 10)[0][-1]) + 1]
    dev = torch.from_numpy(host).cuda()
    off = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.nonzero(dev == 10).flatten() + 1]).contiguous()
    n = off.numel() - 1
    call = (lambda: r.search_longest_extents(dev, off, trim=1)) if side == "search_longest" else (lambda: r.search_extents(dev, off, trim=1))
    start, end = call()
    found = end >= 0
    matched = int((end[found] - start[found]).sum())
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(launches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); call(); b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    med = statistics.median(ms)
    print(json.dumps({"config": kind, "tree": os.path.relpath(tree, ROOT), "side": side, "bytes": int(dev.numel()), "items": n, "found": int(found.sum()),
                      "matched_bytes": matched, "ms": round(med, 4), "TB/s": round(dev.numel() / med / 1e9, 3), "min_ms": round(ms[0], 4),
                      "max_ms": round(ms[-1], 4), "spread": round((ms[-1] - ms[0]) / med, 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", default=os.path.join(ROOT, ".oldtree"))
    ap.add_argument("--launches", type=int, default=15)
    ap.add_argument("--scale", type=float, default=1.0, help="corpus sizes times this (a quick run)")
    ap.add_argument("--child", nargs=5, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        tree, side, kind, pkey, nbytes = a.child
        return child(tree, side, kind, pkey, int(nbytes), max(a.launches, 12))
    assert os.path.exists(os.path.join(a.old, "roaringregex_amd", "librrx.so")), "build the parent commit under %s first" % a.old
    print("expected: search_longest reads every item to its end and the match again, search_items stops at the first hit - where most "
          "items match early the new call is slower: the price of leftmost-longest", flush=True)
    for kind, pkey, nbytes in CONFIGS:
        n = int(nbytes * a.scale) // 4096 * 4096
        for tree, side in ((ROOT, "search_longest"), (a.old, "search_items")) * 2:
            env = dict(os.environ)
            env.pop("RRX_LIB", None)
            rc = subprocess.call([sys.executable, os.path.abspath(__file__), "--launches", str(a.launches), "--child", tree, side, kind, pkey, str(n)],
                                 env=env, timeout=600)
            if rc:                             # a fault or a time limit: nothing more is started on the device
                raise SystemExit("child failed with %d: %s %s %s" % (rc, tree, side, kind))


if __name__ == "__main__":
    main()
