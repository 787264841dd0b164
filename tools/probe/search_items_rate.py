"""rrx_search_extents (a lane per item) beside the two numbers it has to be held against, on the URL, email and keyword-log texts of
bench.py viewed as items (offsets = the line starts, trim 1: the '\\n' is the separator) and on 65536 items of 4 KiB whose only
match lies in the first 100 bytes:

  search_items    this tree: rrx_search_extents on the batch;
  search_corpus   the parent commit: rrx_search_corpus on the same bytes as a corpus, its index built - today's workaround for a
                  string column without '\\n' inside its items, the number to beat or explain;
  contains_lanes  the parent commit: rrx_contains_extents in slices of 65535 items, below the stripe-wise threshold, so every
                  slice runs a lane per item - the same forward walk without offsets and without the walk back: the floor.

The parent's sides run from a second checkout under .oldtree/ (git archive <commit> | tar -x -C .oldtree; build there), alternating
with this tree's, a fresh process each; device events around every launch (every sweep of slices), median and spread of
`--launches` launches (at least twelve) after warm-up.

    python tools/probe/search_items_rate.py [--old .oldtree] [--launches 15] [--scale 1.0]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CONFIGS = (("url", "U2", 1 << 30), ("email", "EMAIL", 1 << 30), ("kwlog", "K1000C", 1 << 30), ("4KiB_items", "EMAIL", 256 << 20))
SLICE = 65535                                  # items per rrx_contains_extents call: one below kItemsStripesMin


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
    if kind == "4KiB_items":
        item = (b"xy z" * 8 + b"a.b@c1 " + b"xy z" * 1024)[:4095] + b"\n"
        host = np.frombuffer(item * (nbytes // 4096), dtype=np.uint8).copy()
    else:
        host = synth.corpus(kind, 1, nbytes, threads=min(len(os.sched_getaffinity(0)), 16))
        host = host[:int(np.nonzero(host == 10)[0][-1]) + 1]
    dev = torch.from_numpy(host).cuda()
    off = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.nonzero(dev == 10).flatten() + 1]).contiguous()
    n = off.numel() - 1

    if side == "search_items":
        call = lambda: r.search_extents(dev, off, trim=1)
        found = int((call()[1] >= 0).sum())
    elif side == "search_corpus":
        corpus = rr.Corpus(dev)
        assert corpus.num_lines == n
        call = lambda: r.search_corpus(corpus)
        found = int((call()[1] >= 0).sum())
    else:
        bits = torch.empty((SLICE + 31) // 32, dtype=torch.int32, device="cuda")
        slices = [off[k:k + SLICE + 1] for k in range(0, n, SLICE)]

        def call():
            for s in slices:
                r.contains_extents_bits(dev, s, trim=1, out=bits)
        found = sum(rr.bitmap_count(r.contains_extents_bits(dev, s, trim=1), s.numel() - 1) for s in slices)
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
    ap.add_argument("--child", nargs=5, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        tree, side, kind, pkey, nbytes = a.child
        return child(tree, side, kind, pkey, int(nbytes), max(a.launches, 12))
    assert os.path.exists(os.path.join(a.old, "roaringregex_amd", "librrx.so")), "build the parent commit under %s first" % a.old
    for kind, pkey, nbytes in CONFIGS:
        n = int(nbytes * a.scale) // 4096 * 4096
        for tree, side in ((ROOT, "search_items"), (a.old, "search_corpus"), (a.old, "contains_lanes")) * 2:
            env = dict(os.environ)
            env.pop("RRX_LIB", None)
            rc = subprocess.call([sys.executable, os.path.abspath(__file__), "--launches", str(a.launches), "--child", tree, side, kind, pkey, str(n)],
                                 env=env, timeout=600)
            if rc:                             # a fault or a time limit: nothing more is started on the device
                raise SystemExit("child failed with %d: %s %s %s" % (rc, tree, side, kind))


if __name__ == "__main__":
    main()
