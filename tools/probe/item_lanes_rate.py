"""The rate of ONE lane-per-item entry in this tree beside the SAME entry of the parent commit - the probe for a change that is
meant to leave these kernels as fast as they were (item_lanes.hpp).  On the URL, email and keyword-log texts of bench.py viewed as
items (offsets = the line starts, trim 1: the '\\n' is the separator):

  match           rrx_match_extents       in slices of 65535 items, below the stripe-wise threshold: every slice runs a lane per item
  contains        rrx_contains_extents    in the same slices
  search          rrx_search_extents      on the whole batch
  search_all      rrx_search_all_extents_count + _fill on the whole batch
  search_longest  rrx_search_longest_extents on the whole batch
  search_all_longest  rrx_search_all_longest_extents_count + _fill on the whole batch (the marks buffer allocated per call, as the
                  Python wrapper does).  The parent has no such entry: its side runs `search_all`, the nearest thing it has - A
                  DIFFERENT QUESTION (matches taken earliest-end-first, no marks, no backward pass over the whole item), so the two
                  sides do not find the same and "within_margin" says how far the new entry is from that yardstick, not whether
                  anything got slower.

  replace         the column with every leftmost-longest match replaced (kernels_replace_items.hip), rep_len 1 and 16: per launch
                  rrx_replace_matches_sizes, rrx_replace_matches_fill (the lists found once, outside the timed window) and the
                  one-call rrx_replace_all_longest_extents (search, scans, sizes and fill, its allocations included), and as the
                  yardstick a device-to-device copy of the column's bytes - the least any writer of a column can cost -, the four
                  alternating inside one process.  The parent has no such entry and plays no part: one child per text, this tree
                  alone; the lines and a summary (fill as a share of the copy's rate) go to `--out` as well.

The parent's side runs from a second checkout under .oldtree/ (git archive <commit> | tar -x -C .oldtree; build there): per text
four children - parent, tree, parent, tree -, a fresh process each; device events around every launch (every sweep of slices),
median and spread of `--launches` launches (at least twelve) after warm-up.  A child that fails ends the run: nothing more is
started on the device.  The last line per text gives the margin - what the parent differs from itself: the larger of the distance
between its two medians and its own spread - and whether each of the tree's medians is within it of the slower parent median.

    python tools/probe/item_lanes_rate.py --entry search [--old .oldtree] [--launches 15] [--scale 1.0]
    python tools/probe/item_lanes_rate.py --entry replace [--launches 15] [--scale 1.0] [--out profiles/replace_items_rate.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CONFIGS = (("url", "U2", 1 << 30), ("email", "EMAIL", 1 << 30), ("kwlog", "K1000C", 1 << 30))
ENTRIES = ("match", "contains", "search", "search_all", "search_longest", "search_all_longest", "replace")
YARDSTICK = {"search_all_longest": "search_all"}   # entries the parent lacks: what its side runs instead
SLICE = 65535                                  # items per call of match / contains: one below kItemsStripesMin


def child(tree, entry, kind, pkey, nbytes, launches):
    sys.path.insert(0, os.path.join(ROOT, "tools"))    # synth and bench.patterns(): the same text and patterns for both sides
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from bench import patterns
    import synth
    sys.path.remove(ROOT)
    sys.path.insert(0, tree)
    import roaringregex_amd as rr
    assert os.path.dirname(os.path.abspath(rr.__file__)).startswith(os.path.abspath(tree)), rr.__file__
    r = rr.RRegex(patterns()[pkey])
    host = synth.corpus(kind, 1, nbytes, threads=min(len(os.sched_getaffinity(0)), 16))
    host = host[:int(np.nonzero(host == 10)[0][-1]) + 1]
    dev = torch.from_numpy(host).cuda()
    off = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.nonzero(dev == 10).flatten() + 1]).contiguous()
    n = off.numel() - 1
    if entry == "replace":
        return replace_child(rr, r, kind, dev, off, n, launches)

    if entry in ("match", "contains"):
        slices = [off[k:k + SLICE + 1] for k in range(0, n, SLICE)]
        if entry == "match":
            out = torch.empty(SLICE, dtype=torch.uint8, device="cuda")
            one = lambda s: r.match_extents(dev, s, trim=1, out=out)
            found = sum(int(one(s).sum()) for s in slices)
        else:
            out = torch.empty((SLICE + 31) // 32, dtype=torch.int32, device="cuda")
            one = lambda s: r.contains_extents_bits(dev, s, trim=1, out=out)
            found = sum(rr.bitmap_count(one(s), s.numel() - 1) for s in slices)

        def call():
            for s in slices:
                one(s)
    elif entry in ("search_all", "search_all_longest"):
        call = (lambda: r.search_all_extents(dev, off, trim=1)) if entry == "search_all" else (lambda: r.search_all_longest_extents(dev, off, trim=1))
        found = int(call()[2].numel())             # (matches in all)
    else:
        call = (lambda: r.search_extents(dev, off, trim=1)) if entry == "search" else (lambda: r.search_longest_extents(dev, off, trim=1))
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
    print(json.dumps({"config": kind, "tree": os.path.relpath(tree, ROOT), "entry": entry, "bytes": int(dev.numel()), "items": n, "found": found,
                      "ms": round(med, 4), "TB/s": round(dev.numel() / med / 1e9, 3), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4),
                      "spread": round((ms[-1] - ms[0]) / med, 4)}), flush=True)


def replace_child(rr, r, kind, dev, off, n, launches):
    """sizes, fill, the one-call form and a device-to-device copy of the column, alternating, per rep_len one JSON line."""
    import ctypes as C
    import torch
    L, s, nbytes = rr._L, rr._stream_ptr(None), int(dev.numel())
    ptr = lambda t: C.c_void_p(t.data_ptr())
    first, start, end = r.search_all_longest_extents_fused(dev, off, trim=1)
    copy_to = torch.empty_like(dev)
    for rep_len in (1, 16):
        rep = bytes(range(65, 65 + rep_len))
        d_rep = torch.frombuffer(bytearray(rep), dtype=torch.uint8).cuda()
        length = torch.empty(n, dtype=torch.int32, device="cuda")
        pos = torch.empty(max(int(start.numel()), 1), dtype=torch.int32, device="cuda")
        sizes = lambda: rr._check(L.rrx_replace_matches_sizes(0, ptr(off), n, 1, ptr(first), ptr(start), ptr(end), rep_len, ptr(length), ptr(pos), s))
        sizes()
        out_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        torch.cumsum(length.to(torch.int64), dim=0, out=out_off[1:])
        total = int(out_off[-1])
        out = torch.empty(total, dtype=torch.uint8, device="cuda")
        fill = lambda: rr._check(L.rrx_replace_matches_fill(0, ptr(dev), ptr(off), n, 1, ptr(first), ptr(end), ptr(pos), ptr(d_rep), rep_len, ptr(out_off),
                                                            ptr(out), s))
        one_off, one_out, tot = torch.empty(n + 1, dtype=torch.int64, device="cuda"), torch.empty(total, dtype=torch.uint8, device="cuda"), C.c_size_t(0)
        one = lambda: rr._check(L.rrx_replace_all_longest_extents(r._h, 0, ptr(dev), ptr(off), n, 1, rep, rep_len, ptr(one_off), ptr(one_out), total,
                                                                  C.byref(tot), s))
        calls = {"copy": lambda: copy_to.copy_(dev), "sizes": sizes, "fill": fill, "one_call": one}
        for _ in range(3):
            for call in calls.values():
                call()
        torch.cuda.synchronize()
        assert tot.value == total and torch.equal(one_out, out) and torch.equal(one_off, out_off), "the one-call form and the two passes differ"
        ms = {k: [] for k in calls}
        for _ in range(launches):
            for k, call in calls.items():                   # alternating: every launch of a kernel has a copy right beside it
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); call(); b.record()
                b.synchronize()
                ms[k].append(a.elapsed_time(b))
        med = {k: statistics.median(v) for k, v in ms.items()}
        line = {"config": kind, "entry": "replace", "rep_len": rep_len, "bytes": nbytes, "items": n, "matches": int(start.numel()), "out_bytes": total}
        for k in calls:
            line[k + "_ms"] = round(med[k], 4)
            line[k + "_spread"] = round((max(ms[k]) - min(ms[k])) / med[k], 4)
        line["copy_GB/s"] = round(nbytes / med["copy"] / 1e6, 1)                    # bytes copied (read and written once each)
        line["fill_GB/s"] = round(total / med["fill"] / 1e6, 1)                     # bytes of the new column written
        line["fill_share_of_copy"] = round((total / med["fill"]) / (nbytes / med["copy"]), 4)
        print(json.dumps(line), flush=True)


def replace_main(a):
    """One child per text, this tree alone; the lines and a summary to a.out."""
    lines = []
    for kind, pkey, nbytes in CONFIGS:
        n = int(nbytes * a.scale) // 4096 * 4096
        env = dict(os.environ)
        env.pop("RRX_LIB", None)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--entry", "replace", "--launches", str(a.launches), "--child", ROOT, kind, pkey, str(n)],
                           env=env, timeout=600, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode:                       # a fault or a time limit: nothing more is started on the device
            raise SystemExit("child failed with %d: replace %s" % (p.returncode, kind))
        lines += [json.loads(x) for x in p.stdout.strip().splitlines()]
    shares = [x["fill_share_of_copy"] for x in lines]
    summary = {"entry": "replace", "launches": max(a.launches, 12), "scale": a.scale, "fill_share_of_copy_min": min(shares), "fill_share_of_copy_max": max(shares),
               "fill_under_a_quarter_of_the_copy": min(shares) < 0.25}
    print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("tools/probe/item_lanes_rate.py --entry replace --launches %d --scale %g: medians of device-event times per launch, the four calls\n"
                "alternating in one process per text; GB/s = bytes of the column written (fill) or copied (copy) per second.\n" % (a.launches, a.scale))
        for x in lines + [summary]:
            f.write(json.dumps(x) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entry", choices=ENTRIES, required=True)
    ap.add_argument("--old", default=os.path.join(ROOT, ".oldtree"))
    ap.add_argument("--launches", type=int, default=15)
    ap.add_argument("--scale", type=float, default=1.0, help="corpus sizes times this (a quick run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replace_items_rate.txt"), help="--entry replace: where the lines and the summary go")
    ap.add_argument("--child", nargs=4, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        tree, kind, pkey, nbytes = a.child
        return child(tree, a.entry, kind, pkey, int(nbytes), max(a.launches, 12))
    if a.entry == "replace":
        return replace_main(a)
    assert os.path.exists(os.path.join(a.old, "roaringregex_amd", "librrx.so")), "build the parent commit under %s first" % a.old
    for kind, pkey, nbytes in CONFIGS:
        n = int(nbytes * a.scale) // 4096 * 4096
        runs = {"parent": [], "tree": []}
        for side, tree in (("parent", a.old), ("tree", ROOT)) * 2:
            env = dict(os.environ)
            env.pop("RRX_LIB", None)
            entry = YARDSTICK.get(a.entry, a.entry) if side == "parent" else a.entry
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--entry", entry, "--launches", str(a.launches), "--child", tree, kind, pkey, str(n)],
                               env=env, timeout=600, stdout=subprocess.PIPE, text=True)
            sys.stdout.write(p.stdout)
            sys.stdout.flush()
            if p.returncode:                   # a fault or a time limit: nothing more is started on the device
                raise SystemExit("child failed with %d: %s %s %s" % (p.returncode, tree, entry, kind))
            runs[side].append(json.loads(p.stdout.strip().splitlines()[-1]))
        if a.entry in YARDSTICK:
            assert len({x["found"] for x in runs["parent"]}) == 1 and len({x["found"] for x in runs["tree"]}) == 1, "a tree does not repeat itself"
            print("# parent side: %s, tree side: %s - a different question, the yardstick is only the nearest thing the parent has" % (YARDSTICK[a.entry], a.entry))
        else:
            assert len({x["found"] for x in runs["parent"] + runs["tree"]}) == 1, "the two trees do not find the same"
        slower = max(x["ms"] for x in runs["parent"])
        margin = max(abs(runs["parent"][0]["ms"] - runs["parent"][1]["ms"]), max(x["spread"] * x["ms"] for x in runs["parent"]))
        print(json.dumps({"config": kind, "entry": a.entry, "parent_ms": [x["ms"] for x in runs["parent"]], "tree_ms": [x["ms"] for x in runs["tree"]],
                          "margin_ms": round(margin, 4), "within_margin": all(x["ms"] <= slower + margin for x in runs["tree"])}), flush=True)


if __name__ == "__main__":
    main()
