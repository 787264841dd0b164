"""rrx_contains_corpus against the entry it replaces (rrx_search_corpus) and its ceiling (rrx_match_corpus of the same pattern) on
the corpora bench.py builds: URL 8 GiB, email and keyword log 1 GiB.  The search and match side run from a second checkout of
the parent commit under .oldtree/ (as tools/probe/ab_oldtree.sh: git archive <commit> | tar -x -C .oldtree; build there), the
contains side from this tree, alternating, a fresh process each; device events around every launch, median and spread of
`--launches` launches (at least twelve) after warm-up.  The text with high bytes is the same corpus with a two-byte UTF-8
character laid over two text bytes in about one line in a hundred.

    python tools/probe/contains_rate.py [--old .oldtree] [--launches 15] [--scale 1.0]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CONFIGS = (("url", "U2", 8 << 30), ("email", "EMAIL", 1 << 30), ("kwlog", "K1000C", 1 << 30))


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

    def timed(call):
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
        return {"ms": round(med, 4), "TB/s": round(nbytes / med / 1e9, 3), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4),
                "spread": round((ms[-1] - ms[0]) / med, 4)}

    out = {}
    variants = (("plain", False), ("utf8", True)) if side == "contains" else (("plain", False),)
    for name, high in variants:
        if high:
            rng = np.random.default_rng(3)
            pos = rng.integers(0, host.size - 1, size=max(int((host == 10).sum()) // 100, 1))
            pos = pos[(host[pos] != 10) & (host[pos + 1] != 10)]
            host[pos] = 0xC3
            host[pos + 1] = 0xA9
        dev = torch.from_numpy(host).cuda()
        c = rr.Corpus(dev)
        if side == "contains":
            bits = r.contains_corpus_bits(c)
            out["contains_" + name] = dict(timed(lambda: r.contains_corpus_bits(c, out=bits)), engine=r.contains_engine_name, states=r.contains_states,
                                           lines=c.num_lines, contained=rr.bitmap_count(bits, c.num_lines))
        else:
            s, e = r.search_corpus(c)
            out["search"] = dict(timed(lambda: r.search_corpus(c)), found=int((s != -1).sum()), lines=c.num_lines)
            bits = r.match_corpus_bits(c)
            torch.cuda.synchronize()
            import time
            time.sleep(0.5)                    # (the background table order, where one is searched for, is in before the timing)
            out["match"] = dict(timed(lambda: r.match_corpus_bits(c, out=bits)), engine=r.engine_name)
        del dev, c
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
        for tree, side in ((a.old, "search"), (ROOT, "contains"), (a.old, "search"), (ROOT, "contains")):
            env = dict(os.environ)
            env.pop("RRX_LIB", None)
            rc = subprocess.call([sys.executable, os.path.abspath(__file__), "--launches", str(a.launches), "--child", tree, side, kind, pkey, str(n)],
                                 env=env, timeout=400)
            if rc:                             # a fault or a time limit: nothing more is started on the device
                raise SystemExit("child failed with %d: %s %s %s" % (rc, tree, side, kind))


if __name__ == "__main__":
    main()
