"""rrx_search_all_extents* (a lane per item, every match) beside the two parent-commit numbers it has to be held against, on the URL,
email and keyword-log texts of bench.py at 1 GiB viewed as items (offsets = the line starts, trim 1: the '\\n' is the separator):

  count           this tree: rrx_search_all_extents_count alone;
  count_fill      this tree: RRegex.search_all_extents - count, the prefix (torch.cumsum and the read-back of the total), fill;
  one_call        this tree: rrx_search_all_extents with match arrays of the exact size (count, device scan, fill, synchronous);
  search_all      the parent commit: rrx_search_all on the same bytes as a corpus, its index built - today's route for a string
                  column without '\\n' inside its items;
  search_extents  the parent commit: rrx_search_extents on the same items - the first match only: the forward walk ends at the
                  first hit, count's goes on to the end of the item.

The parent's sides run from a second checkout under .oldtree/ (git archive <commit> | tar -x -C .oldtree; build there), alternating
with this tree's, a fresh process each; device events around every call, median and spread of `--launches` calls (at least twelve)
after three warm-up calls.

    python tools/probe/search_all_items_rate.py [--old .oldtree] [--launches 15] [--scale 1.0]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CONFIGS = (("url", "U2", 1 << 30), ("email", "EMAIL", 1 << 30), ("kwlog", "K1000C", 1 << 30))
SIDES = (("new", "count"), ("old", "search_extents"), ("new", "count_fill"), ("old", "search_all"), ("new", "one_call"))


def child(tree, side, kind, pkey, nbytes, launches):
    for p in (tree, os.path.join(tree, "tools")):
        sys.path.insert(0, p)
    sys.path.insert(0, ROOT)                   # bench.patterns() only (the same in both trees)
    import ctypes as C
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

    if side == "count":
        count = torch.empty(n, dtype=torch.int32, device="cuda")
        call = lambda: rr._check(rr._L.rrx_search_all_extents_count(r._h, 0, dev.data_ptr(), off.data_ptr(), n, 1, count.data_ptr(), rr._stream_ptr(None)))
        call()
        found = int(count.sum(dtype=torch.int64))
    elif side == "count_fill":
        call = lambda: r.search_all_extents(dev, off, trim=1)
        found = call()[2].numel()
    elif side == "one_call":
        found = r.search_all_extents_fused(dev, off, trim=1)[1].numel()
        call = lambda: r.search_all_extents_fused(dev, off, trim=1, cap=found)
    elif side == "search_all":
        corpus = rr.Corpus(dev)
        assert corpus.num_lines == n
        found = r.search_all_fused(corpus)[1].numel()
        call = lambda: r.search_all_fused(corpus, cap=found)
    else:
        call = lambda: r.search_extents(dev, off, trim=1)
        found = int((call()[1] >= 0).sum())
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
    print(json.dumps({"config": kind, "tree": os.path.relpath(tree, ROOT), "side": side, "bytes": int(dev.numel()), "items": n, "found": found,
                      "ms": round(med, 4), "TB/s": round(dev.numel() / med / 1e9, 3), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4),
                      "spread": round((ms[-1] - ms[0]) / med, 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", default=os.path.join(ROOT, ".oldtree"))
    ap.add_argument("--launches", type=int, default=15)
    ap.add_argument("--scale", type=float, default=1.0, help="corpus sizes times this (a quick run)")
    ap.add_argument("--rounds", type=int, default=2, help="how often every side runs, the sides alternating")
    ap.add_argument("--child", nargs=5, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        tree, side, kind, pkey, nbytes = a.child
        return child(tree, side, kind, pkey, int(nbytes), max(a.launches, 12))
    assert os.path.exists(os.path.join(a.old, "roaringregex_amd", "librrx.so")), "build the parent commit under %s first" % a.old
    for kind, pkey, nbytes in CONFIGS:
        n = int(nbytes * a.scale) // 4096 * 4096
        for which, side in SIDES * a.rounds:
            tree = ROOT if which == "new" else a.old
            env = dict(os.environ)
            env.pop("RRX_LIB", None)
            rc = subprocess.call([sys.executable, os.path.abspath(__file__), "--launches", str(a.launches), "--child", tree, side, kind, pkey, str(n)],
                                 env=env, timeout=600)
            if rc:                             # a fault or a time limit: nothing more is started on the device
                raise SystemExit("child failed with %d: %s %s %s" % (rc, tree, side, kind))


if __name__ == "__main__":
    main()
