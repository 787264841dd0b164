"""rrx_contains_items beside the parent commit's rrx_match_items on the same batch: the URL, email and keyword-log texts of bench.py
viewed as items (offsets = the line starts; trim 1: the '\\n' is the separator, trim 0: it is the item's last byte), batch and index
resident.  The match side runs from a second checkout of the parent commit under .oldtree/ (as tools/probe/ab_oldtree.sh: git
archive <commit> | tar -x -C .oldtree; build there), the contains side from this tree, alternating, a fresh process each; device
events around every launch, median and spread of `--launches` launches (at least twelve) after warm-up.  Both sides name the table
form they ran on: the stripe-wise forms are the same kernels on different tables, a pattern without a contains items table (U2)
runs a lane per item.

The lane-per-item kernel beside the parent's match_extents_kernel: batches indexed with trim 2 never admit the stripe-wise kernels,
so both entries run a lane per item on them - the email text (short items), and 65536 items of 4 KiB whose only match lies in the
first 100 bytes (contains stops reading there; the match side reads every item to its end with a pattern that accepts it).

    python tools/probe/contains_items_rate.py [--old .oldtree] [--launches 15] [--scale 1.0]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CONFIGS = (("url", "U2", 1 << 30), ("email", "EMAIL", 1 << 30), ("kwlog", "K1000C", 1 << 30), ("lanes", "EMAIL", 256 << 20))
WHOLE_ITEM = "[a-z.@1 ]*"                      # accepts every 4 KiB item of the "lanes" config: the match side reads them whole


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

    def timed(call, moved):
        for _ in range(4):
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
        return {"ms": round(med, 4), "TB/s": round(moved / med / 1e9, 3), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4),
                "spread": round((ms[-1] - ms[0]) / med, 4)}

    def run(name, reg, dev, off, trim, out):
        items = rr.Items(dev, off, trim=trim)
        n = items.num_items
        if side == "contains":
            bits = reg.contains_items_bits(items)
            # (the byte-stride items table holds at most 125 rows: 16-bit row offsets)
            form = ("lane per item" if not items.stripe_wise else "stride-2 items table" if trim == 1 and reg.program(18) is not None
                    else "byte-stride items table" if reg.contains_states <= 125 else "lane per item")
            out[name] = dict(timed(lambda: reg.contains_items_bits(items, out=bits), dev.numel()), form=form, states=reg.contains_states, items=n,
                             contained=rr.bitmap_count(bits, n))
        else:
            acc = reg.match_items(items)
            form = ("stride-2 items table" if trim == 1 and reg.program(15) is not None else "byte-stride items table") if items.stripe_wise else "lane per item"
            out[name] = dict(timed(lambda: reg.match_items(items, out=acc), dev.numel()), form=form, engine=reg.engine_name, items=n, accepted=int(acc.sum()))

    out = {}
    if kind == "lanes":
        host = synth.corpus("email", 1, nbytes, threads=min(len(os.sched_getaffinity(0)), 16))
        host = host[:int(np.nonzero(host == 10)[0][-1]) + 1]
        dev = torch.from_numpy(host).cuda()
        off = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.nonzero(dev == 10).flatten() + 1]).contiguous()
        run("short_items_trim2", r, dev, off, 2, out)
        del dev, off
        item = (b"xy z" * 8 + b"a.b@c1 " + b"xy z" * 1024)[:4094] + b";;"
        assert len(item) == 4096
        dev = torch.from_numpy(np.frombuffer(item * 65536, dtype=np.uint8).copy()).cuda()
        off = (torch.arange(65537, dtype=torch.int64, device="cuda") * 4096).contiguous()
        run("4KiB_items_hit_in_first_100_bytes_trim2", r if side == "contains" else rr.RRegex(WHOLE_ITEM), dev, off, 2, out)
    else:
        host = synth.corpus(kind, 1, nbytes, threads=min(len(os.sched_getaffinity(0)), 16))
        host = host[:int(np.nonzero(host == 10)[0][-1]) + 1]
        dev = torch.from_numpy(host).cuda()
        off = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.nonzero(dev == 10).flatten() + 1]).contiguous()
        for trim in (1, 0):
            run("trim%d" % trim, r, dev, off, trim, out)
    print(json.dumps({"config": kind, "tree": os.path.relpath(tree, ROOT), "side": side, "bytes": nbytes, **out}), flush=True)


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
        for tree, side in ((a.old, "match"), (ROOT, "contains"), (a.old, "match"), (ROOT, "contains")):
            env = dict(os.environ)
            env.pop("RRX_LIB", None)
            rc = subprocess.call([sys.executable, os.path.abspath(__file__), "--launches", str(a.launches), "--child", tree, side, kind, pkey, str(n)],
                                 env=env, timeout=400)
            if rc:                             # a fault or a time limit: nothing more is started on the device
                raise SystemExit("child failed with %d: %s %s %s" % (rc, tree, side, kind))


if __name__ == "__main__":
    main()
