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

  extract_group   rrx_extract_group_longest_extents (the fused form: rrx_search_longest_extents, then the longest split point once per
                  part that is there, in place; marks and result arrays allocated once, outside the timed window) for group 1 of the
                  text's pattern - the e-mail pattern with its domain in parentheses.  The parent has no such entry: its side runs
                  `search_longest` on the same pattern and the same items - the part of the work that exists already -, both sides
                  must find a match in the same number of items, and the last line gives the ratio of the two medians.

  replace         the column with every leftmost-longest match replaced (kernels_replace_items.hip), rep_len 1 and 16: per launch
                  rrx_replace_matches_sizes, rrx_replace_matches_fill (the lists found once, outside the timed window) and the
                  one-call rrx_replace_all_longest_extents (search, scans, sizes and fill, its allocations included), and as the
                  yardstick a device-to-device copy of the column's bytes - the least any writer of a column can cost -, the four
                  alternating inside one process.  The parent has no such entry and plays no part: one child per text, this tree
                  alone; the lines and a summary (fill as a share of the copy's rate) go to `--out` as well.

  pieces          the list<binary> columns of extract_all and split (kernels_pieces_items.hip): per launch a device-to-device copy of
                  the column's bytes, rrx_replace_matches_fill with rep_len 0, rrx_pieces_fill on GAPS - which writes the identical
                  bytes: this pair is the A/B -, rrx_pieces_fill on MATCHES, rrx_pieces_sizes (GAPS) and both one-call forms, the
                  seven alternating inside one process, in three rounds of `--launches` launches: the margin of the A/B is the
                  baseline's own spread, min to max of its three medians.  Per text one child, this tree alone; a fourth child
                  runs the SKEWED batch: the URL text (a quarter longer) whose first 64 items are merged lines of 16 MiB each - for
                  replace's fill one wave's work, which is why that child makes two rounds of two launches only.

  one_call        the entries that count, scan, read a total back and fill inside one call - rrx_search_all_extents,
                  rrx_search_all_longest_extents, rrx_replace_all_longest_extents (rep_len 1), rrx_extract_all_longest_extents and
                  rrx_split_longest_extents - on the first 4096 lines of the e-mail text: a batch so small that a call is its
                  launches' latencies, its allocations and its synchronisations, which is what a change of the host code can move.
                  Both sides run THIS tree's Python and differ in the library alone: the parent's children load
                  .oldtree/roaringregex_amd/librrx.so through RRX_LIB.  Exact caps (learnt by a call with cap 0), the five calls
                  alternating, host time per call - each returns behind its last synchronise -, the same four children and the same
                  margin as below, per entry; the lines go to `--out` as well.

  replace_groups  regexp_replace with group references (kernels_replace_template_items.hip, longest_split_list_kernel) on the e-mail
                  text, the pattern with its domain in parentheses: the one-call rrx_replace_groups_longest_extents with the
                  templates \\0, a literal and \\1 beside rrx_replace_all_longest_extents with the same literal - the parent commit's
                  entry, its code untouched in this tree - and, to say where the time goes, the stages behind them on lists found
                  once: rrx_replace_matches_sizes / _fill (the literal), rrx_replace_template_sizes / _fill with the template literal
                  and with \\1, and rrx_group_spans_list_extents; all alternating inside one process.  One child, this tree alone;
                  the lines and a summary (what a group reference costs over the literal path) go to `--out` as well.

  multi_contains  which of K keywords every line of the keyword-log text contains (kernels_multi_items.hip), K = 1, 4, 16 and 32:
                  rrx_multi_contains_items on a set of K keywords beside what the parent commit offers for the same question - K calls
                  of rrx_contains_items, one per keyword, on the same indexed batch (its code untouched in this tree) -, the two
                  alternating inside one process, the masks checked against the K bitmaps bit for bit.  One child, this tree alone;
                  the lines and a summary (the smallest K at which the set wins, if any) go to `--out` as well.

  multi_contains_corpus  the same question about the LINES of the keyword-log text held as an rrx_corpus (kernels_multi_corpus.hip, a
                  lane per stripe), K = 1, 4, 16 and 32, three ways: (a) corpus = one rrx_multi_contains_corpus, (b) singles = K calls
                  of rrx_contains_corpus, (c) items = rrx_multi_contains_items on an indexed batch over the same lines - the only
                  one-walk way the parent commit offers -, the three alternating inside one process; (a)'s masks must equal (c)'s
                  word for word and their planes (b)'s bitmaps.  A difference of two medians counts only beyond the sum of the two
                  spreads [ms].  One child, this tree alone; the lines and a summary go to `--out` as well.

  search_longest_corpus  the leftmost-longest match of every LINE of the keyword-log and the e-mail text held as an rrx_corpus
                  (kernels_search_longest_corpus.hip, a lane per stripe), three ways alternating inside one process: (a) corpus =
                  rrx_search_longest_corpus, (b) items = rrx_search_longest_items on an indexed batch over the same lines - the
                  parent commit's code and the nearest thing it has -, (c) first = rrx_search_corpus, the other question on the
                  same shape, a yardstick for what the two passes cost; (a) must equal (b) word for word before anything is timed.
                  A difference of two medians counts only beyond the sum of the two spreads [ms].  One child per text, this tree
                  alone; the lines go to `--out` as well.

  filter          the rows a bitmap selects, written as a new column (kernels_filter.hip) on the keyword-log and the e-mail text: a
                  device-to-device copy of the column beside rrx_pieces_fill of EVERY line (the invert of an all-zero bitmap) - the
                  fill's share of a plain copy -, then on the pattern's real contains bitmap rrx_bitmap_rank, rrx_filter_sizes,
                  rrx_filter_corpus_sizes and rrx_pieces_fill one by one, the two generic routes whole, the route a caller took
                  before with torch (rrx_bitmap_to_bytes, nonzero, index, cumsum, rrx_pieces_fill), contains alone and the three
                  one-call forms rrx_filter_contains_*; every route must give the same column before anything is timed, all calls
                  alternate inside one process.  A difference of two medians counts only beyond the sum of the two spreads [ms].
                  It takes no parent: one child per text, this tree alone; the lines go to `--out` as well.

A yardstick stands in only for a parent that lacks the entry (its wrapper shows it): a later parent runs the entry itself, and both
sides must find the same.

The parent's side runs from a second checkout under .oldtree/ (git archive <commit> | tar -x -C .oldtree; build there): per text
four children - parent, tree, parent, tree -, a fresh process each; device events around every launch (every sweep of slices),
median and spread of `--launches` launches (at least twelve) after warm-up.  A child that fails ends the run: nothing more is
started on the device.  The last line per text gives the margin - what the parent differs from itself: the larger of the distance
between its two medians and its own spread - and whether each of the tree's medians is within it of the slower parent median.

    python tools/probe/item_lanes_rate.py --entry search [--old .oldtree] [--launches 15] [--scale 1.0]
    python tools/probe/item_lanes_rate.py --entry replace [--launches 15] [--scale 1.0] [--out profiles/replace_items_rate.txt]
    python tools/probe/item_lanes_rate.py --entry pieces [--launches 15] [--scale 1.0] [--out profiles/pieces_items_rate.txt]
    python tools/probe/item_lanes_rate.py --entry one_call [--old .oldtree] [--launches 15] [--out profiles/one_call_items_rate.txt]
    python tools/probe/item_lanes_rate.py --entry replace_groups [--launches 15] [--scale 1.0] [--out profiles/replace_template_items_rate.txt]
    python tools/probe/item_lanes_rate.py --entry multi_contains [--launches 15] [--scale 1.0] [--out profiles/multi_contains_items_rate.txt]
    python tools/probe/item_lanes_rate.py --entry multi_contains_corpus [--launches 15] [--scale 1.0] [--out profiles/multi_contains_corpus_rate.txt]
    python tools/probe/item_lanes_rate.py --entry search_longest_corpus [--launches 15] [--scale 1.0] [--out profiles/search_longest_corpus_rate.txt]
    python tools/probe/item_lanes_rate.py --entry filter [--launches 15] [--scale 1.0] [--out profiles/filter_rate.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CONFIGS = (("url", "U2", 1 << 30), ("email", "EMAIL", 1 << 30), ("kwlog", "K1000C", 1 << 30))
ENTRIES = ("match", "contains", "search", "search_all", "search_longest", "search_all_longest", "extract_group", "replace", "pieces", "one_call", "replace_groups",
           "multi_contains", "multi_contains_corpus", "search_longest_corpus", "filter")
MULTI_KS = (1, 4, 16, 32)                      # --entry multi_contains: the sizes of the keyword sets
MULTI_KEYWORDS = ["k%d" % (61 * j + 17) for j in range(32)]     # k17, k78, ... k1908: the text's tokens are k1 .. k2000
GROUPED = {"EMAIL": r"[A-Za-z0-9._]+@([A-Za-z0-9.]+)"}      # --entry extract_group: the patterns that need a group put in; group 1 everywhere
SKEW_ITEMS, SKEW_ITEM_BYTES = 64, 16 << 20     # the skewed batch of --entry pieces: its first 64 items are merged lines of 16 MiB or more
YARDSTICK = {"search_all_longest": "search_all", "extract_group": "search_longest"}   # entries the parent lacks: what its side runs instead
SAME_ITEMS = ("extract_group",)                # ... of them those whose yardstick answers for the same items: `found` agrees
NEWER = {"search_all_longest": "def search_all_longest_extents", "extract_group": "class RGroup"}     # how a parent's wrapper shows that it has the entry
SLICE = 65535                                  # items per call of match / contains: one below kItemsStripesMin
ONE_CALL_ITEMS, ONE_CALL_TEXT = 4096, ("email", "EMAIL", 1 << 20)      # --entry one_call: the batch, and the text it is the head of
ONE_CALL_ENTRIES = ("search_all", "search_all_longest", "replace_all_longest", "extract_all_longest", "split_longest")


def child(tree, entry, kind, pkey, nbytes, launches):
    skew = kind.endswith("-skewed")
    kind = kind.split("-")[0]
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
    grouped = pkey.endswith("+group")              # (--entry extract_group: both sides on the pattern as that entry takes it)
    pkey = pkey.split("+")[0]
    pattern = GROUPED.get(pkey, patterns()[pkey]) if grouped else patterns()[pkey]
    if entry == "replace_groups":
        pattern = GROUPED[pkey]
    r = rr.RGroup(pattern, 1) if entry in ("extract_group", "replace_groups") else rr.RRegex(pattern)
    host = synth.corpus(kind, 1, nbytes, threads=min(len(os.sched_getaffinity(0)), 16))
    host = host[:int(np.nonzero(host == 10)[0][-1]) + 1]
    dev = torch.from_numpy(host).cuda()
    off = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.nonzero(dev == 10).flatten() + 1]).contiguous()
    n = off.numel() - 1
    if entry == "replace":
        return replace_child(rr, r, kind, dev, off, n, launches)
    if entry == "pieces":
        return pieces_child(rr, r, kind, dev, off, launches, skew)
    if entry == "one_call":
        return one_call_child(rr, r, kind, dev, off, launches)
    if entry == "replace_groups":
        return replace_groups_child(rr, r, kind, dev, off, n, launches)
    if entry == "multi_contains":
        return multi_contains_child(rr, kind, dev, off, n, launches)
    if entry == "multi_contains_corpus":
        return multi_contains_corpus_child(rr, kind, dev, off, n, launches)
    if entry == "search_longest_corpus":
        return search_longest_corpus_child(rr, r, kind, dev, off, n, launches)
    if entry == "filter":
        return filter_child(rr, r, kind, dev, off, n, launches)

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
    elif entry == "extract_group":
        out = (torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda"))
        marks = torch.empty(rr._L.rrx_search_all_longest_marks_words(dev.numel(), n), dtype=torch.int32, device="cuda")
        call = lambda: r.extract_extents(dev, off, trim=1, out=out, marks=marks)
        found = int((call()[1] >= 0).sum())
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


REPLACE_GROUPS_LITERAL = b"<dom>"


def replace_groups_child(rr, g, kind, dev, off, n, launches):
    """The four one-call forms and the stages behind them, alternating; one JSON line."""
    import ctypes as C
    import torch
    L, s, nbytes, lit = rr._L, rr._stream_ptr(None), int(dev.numel()), REPLACE_GROUPS_LITERAL
    ptr = lambda t: C.c_void_p(t.data_ptr())
    r = g.regex
    first, start, end = r.search_all_longest_extents_fused(dev, off, trim=1)
    nmatches = int(start.numel())
    handles = rr._group_handles([g])
    templates = {"whole": rr.Template(rb"\0"), "literal": rr.Template(lit), "group": rr.Template(rb"\1")}
    calls, totals, outs = {}, {}, {}
    one_off, tot = torch.empty(n + 1, dtype=torch.int64, device="cuda"), C.c_size_t(0)
    rr._check(L.rrx_replace_all_longest_extents(r._h, 0, ptr(dev), ptr(off), n, 1, lit, len(lit), ptr(one_off), None, 0, C.byref(tot), s))
    totals["parent_literal"] = tot.value
    for k, tpl in templates.items():
        rr._check(L.rrx_replace_groups_longest_extents(handles, 1, tpl._h, 0, ptr(dev), ptr(off), n, 1, ptr(one_off), None, 0, C.byref(tot), s))
        totals[k] = tot.value
    assert totals["literal"] == totals["parent_literal"] and totals["whole"] == nbytes - n, totals
    one_out = torch.empty(max(totals.values()), dtype=torch.uint8, device="cuda")
    calls["one_call_parent_literal"] = lambda: rr._check(L.rrx_replace_all_longest_extents(r._h, 0, ptr(dev), ptr(off), n, 1, lit, len(lit), ptr(one_off),
                                                                                           ptr(one_out), one_out.numel(), C.byref(tot), s))
    for k, tpl in templates.items():
        calls["one_call_" + k] = (lambda tpl=tpl: rr._check(L.rrx_replace_groups_longest_extents(handles, 1, tpl._h, 0, ptr(dev), ptr(off), n, 1, ptr(one_off),
                                                                                                 ptr(one_out), one_out.numel(), C.byref(tot), s)))
    # the stages, on the lists found once
    words = L.rrx_search_all_longest_marks_words(nbytes, n)
    marks = torch.empty(words, dtype=torch.int32, device="cuda")
    ref_start, ref_end = torch.empty(max(nmatches, 1), dtype=torch.int32, device="cuda"), torch.empty(max(nmatches, 1), dtype=torch.int32, device="cuda")
    length, pos = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(max(nmatches, 1), dtype=torch.int32, device="cuda")
    d_lit = torch.frombuffer(bytearray(lit), dtype=torch.uint8).cuda()
    calls["list_spans"] = lambda: rr._check(L.rrx_group_spans_list_extents(g._h, 0, ptr(dev), ptr(off), n, 1, ptr(first), ptr(start), ptr(end), ptr(marks), words,
                                                                           ptr(ref_start), ptr(ref_end), s))
    calls["list_spans"]()
    stage_off, stage_out = {}, {}

    def prefix(key):
        stage_off[key] = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        torch.cumsum(length.to(torch.int64), dim=0, out=stage_off[key][1:])
        stage_out[key] = torch.empty(int(stage_off[key][-1]), dtype=torch.uint8, device="cuda")
    calls["sizes_parent_literal"] = lambda: rr._check(L.rrx_replace_matches_sizes(0, ptr(off), n, 1, ptr(first), ptr(start), ptr(end), len(lit), ptr(length), ptr(pos), s))
    calls["sizes_parent_literal"]()
    prefix("parent_literal")
    pos_lit = pos.clone()
    calls["fill_parent_literal"] = lambda: rr._check(L.rrx_replace_matches_fill(0, ptr(dev), ptr(off), n, 1, ptr(first), ptr(end), ptr(pos_lit), ptr(d_lit), len(lit),
                                                                                ptr(stage_off["parent_literal"]), ptr(stage_out["parent_literal"]), s))
    for k in ("literal", "group"):
        tpl = templates[k]
        sizes = (lambda tpl=tpl: rr._check(L.rrx_replace_template_sizes(0, ptr(off), n, 1, ptr(first), ptr(start), ptr(end), tpl._h, ptr(ref_start), ptr(ref_end),
                                                                        max(nmatches, 1), ptr(length), ptr(pos), s)))
        sizes()
        prefix(k)
        pos_k = pos.clone()
        calls["sizes_" + k] = sizes
        calls["fill_" + k] = (lambda tpl=tpl, k=k, pos_k=pos_k: rr._check(L.rrx_replace_template_fill(
            0, ptr(dev), ptr(off), n, 1, ptr(first), ptr(start), ptr(end), ptr(pos_k), tpl._h, ptr(ref_start), ptr(ref_end), max(nmatches, 1), ptr(stage_off[k]),
            ptr(stage_out[k]), s)))
    for _ in range(3):
        for call in calls.values():
            call()
    torch.cuda.synchronize()
    assert torch.equal(stage_out["literal"], stage_out["parent_literal"]) and torch.equal(stage_off["literal"], stage_off["parent_literal"]), \
        "the template literal and the literal entries differ"
    assert int(stage_off["group"][-1]) == totals["group"]
    ms = {k: [] for k in calls}
    for _ in range(launches):
        for k, call in calls.items():                   # alternating: every call has the parent's literal path right beside it
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); call(); b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    med = {k: statistics.median(v) for k, v in ms.items()}
    line = {"config": kind, "entry": "replace_groups", "bytes": nbytes, "items": n, "matches": nmatches, "out_bytes": totals}
    for k in calls:
        line[k + "_ms"] = round(med[k], 4)
        line[k + "_spread"] = round((max(ms[k]) - min(ms[k])) / med[k], 4)
    line["one_call_group_over_parent_literal"] = round(med["one_call_group"] / med["one_call_parent_literal"], 4)
    line["one_call_template_literal_over_parent_literal"] = round(med["one_call_literal"] / med["one_call_parent_literal"], 4)
    line["fill_group_GB/s"] = round(totals["group"] / med["fill_group"] / 1e6, 1)
    line["fill_parent_literal_GB/s"] = round(totals["parent_literal"] / med["fill_parent_literal"] / 1e6, 1)
    print(json.dumps(line), flush=True)


def multi_contains_child(rr, kind, dev, off, n, launches):
    """Per K the set's one call and the K single-pattern calls on one indexed batch, alternating; one JSON line per K."""
    import torch
    nbytes = int(dev.numel())
    items = rr.Items(dev, off, trim=1)
    regs = [rr.RRegex(p) for p in MULTI_KEYWORDS]
    bits = [torch.empty((n + 31) // 32, dtype=torch.int32, device="cuda") for _ in regs]
    masks = torch.empty(n, dtype=torch.int32, device="cuda")
    for k_set in MULTI_KS:
        m = rr.RMulti(MULTI_KEYWORDS[:k_set])

        def singles(k_set=k_set):
            for r, b in zip(regs[:k_set], bits):
                r.contains_items_bits(items, out=b)
        calls = {"multi": lambda m=m: m.contains_items(items, out=masks), "singles": singles}
        for _ in range(3):
            for call in calls.values():
                call()
        torch.cuda.synchronize()
        for k in range(k_set):
            assert torch.equal(m.plane(masks, k), bits[k]), "the set and keyword %d differ" % k
        counts = m.counts(masks).cpu().tolist()
        ms = {k: [] for k in calls}
        for _ in range(launches):
            for k, call in calls.items():                   # alternating: every call of the set has the K single calls right beside it
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); call(); b.record()
                b.synchronize()
                ms[k].append(a.elapsed_time(b))
        med = {k: statistics.median(v) for k, v in ms.items()}
        line = {"config": kind, "entry": "multi_contains", "K": k_set, "bytes": nbytes, "items": n, "groups": m.groups,
                "rows": [m.group_states(g) for g in range(m.groups)], "stripe_wise_singles": bool(items.stripe_wise), "found": sum(counts)}
        for k in calls:
            line[k + "_ms"] = round(med[k], 4)
            line[k + "_spread"] = round((max(ms[k]) - min(ms[k])) / med[k], 4)
            line[k + "_TB/s"] = round(nbytes / med[k] / 1e9, 3)            # bytes of the column per second of the whole question
        line["multi_over_singles"] = round(med["multi"] / med["singles"], 4)
        print(json.dumps(line), flush=True)


def multi_contains_corpus_child(rr, kind, dev, off, n, launches):
    """Per K the set's one call on the corpus, the K single-pattern calls on the corpus and the set's call on the indexed batch of the
    same lines, alternating; one JSON line per K."""
    import torch
    nbytes = int(dev.numel())
    corpus = rr.Corpus(dev)
    assert corpus.num_lines == n
    items = rr.Items(dev, off, trim=1)
    regs = [rr.RRegex(p) for p in MULTI_KEYWORDS]
    bits = [torch.empty((n + 31) // 32, dtype=torch.int32, device="cuda") for _ in regs]
    masks, item_masks = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    for k_set in MULTI_KS:
        m = rr.RMulti(MULTI_KEYWORDS[:k_set])

        def singles(k_set=k_set):
            for r, b in zip(regs[:k_set], bits):
                r.contains_corpus_bits(corpus, out=b)
        calls = {"corpus": lambda m=m: m.contains_corpus(corpus, out=masks), "singles": singles, "items": lambda m=m: m.contains_items(items, out=item_masks)}
        masks.fill_(0x5A5A5A5A)
        for _ in range(3):
            for call in calls.values():
                call()
        torch.cuda.synchronize()
        assert torch.equal(masks, item_masks), "the corpus form and the items form differ"
        for k in range(k_set):
            assert torch.equal(m.plane(masks, k), bits[k]), "the set and keyword %d differ" % k
        counts = m.counts(masks).cpu().tolist()
        ms = {k: [] for k in calls}
        for _ in range(launches):
            for k, call in calls.items():                   # alternating: every call has the other two right beside it
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); call(); b.record()
                b.synchronize()
                ms[k].append(a.elapsed_time(b))
        med = {k: statistics.median(v) for k, v in ms.items()}
        spread = {k: max(v) - min(v) for k, v in ms.items()}
        line = {"config": kind, "entry": "multi_contains_corpus", "K": k_set, "bytes": nbytes, "lines": n, "stripe": corpus.stripe, "groups": m.groups,
                "rows": [m.group_states(g) for g in range(m.groups)], "stripe_wise_items": bool(items.stripe_wise), "found": sum(counts)}
        for k in calls:
            line[k + "_ms"] = round(med[k], 4)
            line[k + "_spread"] = round(spread[k] / med[k], 4)
            line[k + "_spread_ms"] = round(spread[k], 4)
            line[k + "_TB/s"] = round(nbytes / med[k] / 1e9, 3)            # bytes of the text per second of the whole question
        line["corpus_over_items"] = round(med["corpus"] / med["items"], 4)
        line["corpus_over_singles"] = round(med["corpus"] / med["singles"], 4)
        for other in ("items", "singles"):                  # a difference counts only beyond the sum of the two spreads
            line["corpus_beats_" + other] = bool(med[other] - med["corpus"] > spread[other] + spread["corpus"])
            line[other + "_beats_corpus"] = bool(med["corpus"] - med[other] > spread[other] + spread["corpus"])
        print(json.dumps(line), flush=True)


def search_longest_corpus_child(rr, r, kind, dev, off, n, launches):
    """The leftmost-longest search of every line three ways, alternating: (a) corpus = rrx_search_longest_corpus on the text as an
    rrx_corpus, (b) items = rrx_search_longest_items on an indexed batch over the same lines (trim 1), (c) first = rrx_search_corpus,
    the other question on the same corpus; one JSON line."""
    import torch
    nbytes = int(dev.numel())
    corpus = rr.Corpus(dev)
    assert corpus.num_lines == n
    items = rr.Items(dev, off, trim=1)
    out = {k: (torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")) for k in ("corpus", "items", "first")}
    stream = rr._stream_ptr(None)
    ptrs = {k: (s.data_ptr(), e.data_ptr()) for k, (s, e) in out.items()}
    calls = {"corpus": lambda: rr._check(rr._L.rrx_search_longest_corpus(r._h, corpus._h, *ptrs["corpus"], stream)),
             "items": lambda: rr._check(rr._L.rrx_search_longest_items(r._h, items._h, *ptrs["items"], stream)),
             "first": lambda: rr._check(rr._L.rrx_search_corpus(r._h, corpus._h, *ptrs["first"], stream))}
    for t in out["corpus"]:
        t.fill_(0x5A5A5A5A)
    for _ in range(3):
        for call in calls.values():
            call()
    torch.cuda.synchronize()
    assert torch.equal(out["corpus"][0], out["items"][0]) and torch.equal(out["corpus"][1], out["items"][1]), "the corpus form and the items form differ"
    found = out["corpus"][1] >= 0
    assert torch.equal(out["first"][1] >= 0, found), "the leftmost-longest search and the first-match search find different lines"
    ms = {k: [] for k in calls}
    for _ in range(launches):
        for k, call in calls.items():                       # alternating: every call has the other two right beside it
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); call(); b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in ms.items()}
    line = {"config": kind, "entry": "search_longest_corpus", "bytes": nbytes, "lines": n, "stripe": corpus.stripe, "found": int(found.sum()),
            "matched_bytes": int((out["corpus"][1] - out["corpus"][0])[found].sum())}
    for k in calls:
        line[k + "_ms"] = round(med[k], 4)
        line[k + "_spread"] = round(spread[k] / med[k], 4)
        line[k + "_spread_ms"] = round(spread[k], 4)
        line[k + "_TB/s"] = round(nbytes / med[k] / 1e9, 3)
    line["corpus_over_items"] = round(med["corpus"] / med["items"], 4)
    line["corpus_over_first"] = round(med["corpus"] / med["first"], 4)
    line["corpus_beats_items"] = bool(med["items"] - med["corpus"] > spread["items"] + spread["corpus"])     # beyond the sum of the two spreads
    line["items_beats_corpus"] = bool(med["corpus"] - med["items"] > spread["items"] + spread["corpus"])
    print(json.dumps(line), flush=True)


def filter_child(rr, r, kind, dev, off, n, launches):
    """The rows a bitmap selects, written as a new column (rrx_bitmap_rank, rrx_filter_sizes, rrx_filter_corpus_sizes, rrx_pieces_fill,
    rrx_filter_contains_*), all alternating: (a) copy = a device-to-device copy of the column, fill_all = rrx_pieces_fill of EVERY line
    (the invert of an all-zero bitmap; the output is the text); (b) on the pattern's real contains bitmap: rank, items_select,
    corpus_select and fill one by one, the two generic routes whole (rank, select, torch.cumsum, the size read back, fill), the route a
    caller takes today with torch (rrx_bitmap_to_bytes, nonzero, index, cumsum, the size read back, rrx_pieces_fill), contains alone on
    the corpus and on the indexed batch, and the three one-call forms; one JSON line."""
    import ctypes as C
    import torch
    L, stream = rr._L, rr._stream_ptr(None)
    nbytes = int(dev.numel())
    corpus = rr.Corpus(dev)
    assert corpus.num_lines == n
    items = rr.Items(dev, off, trim=1)
    nw = (n + 31) // 32
    p = lambda t: C.c_void_p(t.data_ptr())
    rank_words = L.rrx_bitmap_rank_words(n)
    rank = torch.empty(rank_words, dtype=torch.int64, device="cuda")
    row, length, src = (torch.empty(n, dtype=torch.int64, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda"),
                        torch.empty(n, dtype=torch.int64, device="cuda"))
    out_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    out, copy_to = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    as_bytes = torch.empty((n + 15) // 16 * 16, dtype=torch.uint8, device="cuda")

    def do_rank(bits, invert):
        rr._check(L.rrx_bitmap_rank(0, p(bits), n, invert, p(rank), rank_words, stream))

    def do_select(bits, invert, keep, of_items):
        if of_items:
            rr._check(L.rrx_filter_sizes(0, p(off), n, 1, p(bits), invert, p(rank), p(row), p(length), p(src), stream))
        else:
            rr._check(L.rrx_filter_corpus_sizes(corpus._h, p(bits), invert, keep, p(rank), p(row), p(length), p(src), stream))

    def prefix(nsel):
        torch.cumsum(length[:nsel].to(torch.int64) & 0xFFFFFFFF, dim=0, out=out_off[1:nsel + 1])
        return int(out_off[nsel].item())

    def do_fill(nsel):
        rr._check(L.rrx_pieces_fill(0, p(dev), p(src), p(out_off), nsel, p(out), stream))

    def route(bits, of_items):
        do_rank(bits, 0)
        nsel = int(rank[nw].item())
        do_select(bits, 0, 0, of_items)
        total = prefix(nsel)
        do_fill(nsel)
        return nsel, total

    def torch_route(bits):
        rr._check(L.rrx_bitmap_to_bytes(0, p(bits), n, p(as_bytes), stream))
        rows = torch.nonzero(as_bytes[:n]).flatten()
        nsel = rows.numel()
        start = off[rows]
        src[:nsel] = start
        torch.cumsum(off[rows + 1] - 1 - start, dim=0, out=out_off[1:nsel + 1])
        total = int(out_off[nsel].item())
        do_fill(nsel)
        return nsel, total

    # (a) every line selected, its newline kept: the output is the text
    zeros = torch.zeros(nw, dtype=torch.int32, device="cuda")
    do_rank(zeros, 1)
    assert int(rank[nw].item()) == n
    do_select(zeros, 1, 1, False)
    assert prefix(n) == nbytes
    do_fill(n)
    torch.cuda.synchronize()
    assert torch.equal(out, dev), "every line selected with its newline is not the text"
    all_src, all_off = src.clone(), out_off.clone()

    # (b) the pattern's contains bitmap
    bits = r.contains_corpus_bits(corpus).clone()
    assert torch.equal(r.contains_items_bits(items), bits), "contains on the corpus and on the indexed batch differ"
    nsel, total = route(bits, True)
    torch.cuda.synchronize()
    want_rows, want_off, want_out = row[:nsel].clone(), out_off[:nsel + 1].clone(), out[:total].clone()
    for name, got in (("corpus", route(bits, False)), ("torch", torch_route(bits))):
        torch.cuda.synchronize()
        assert got == (nsel, total) and torch.equal(out_off[:nsel + 1], want_off) and torch.equal(out[:total], want_out), "the %s route differs from the items route" % name
    assert torch.equal(row[:nsel], want_rows)
    nrows, tot = C.c_size_t(0), C.c_size_t(0)
    one_tail = lambda: (p(row), p(out_off), n, p(out), nbytes, C.byref(nrows), C.byref(tot), stream)
    one = {"one_call_extents": lambda: rr._check(L.rrx_filter_contains_extents(r._h, 0, p(dev), p(off), n, 1, 0, *one_tail())),
           "one_call_items": lambda: rr._check(L.rrx_filter_contains_items(r._h, items._h, 0, *one_tail())),
           "one_call_corpus": lambda: rr._check(L.rrx_filter_contains_corpus(r._h, corpus._h, 0, 0, *one_tail()))}
    for name, call in one.items():
        call()
        torch.cuda.synchronize()
        assert (nrows.value, tot.value) == (nsel, total) and torch.equal(out[:total], want_out) and torch.equal(row[:nsel], want_rows), name + " differs from the items route"

    def select_alone(of_items):
        do_select(bits, 0, 0, of_items)

    def fill_all():
        rr._check(L.rrx_pieces_fill(0, p(dev), p(all_src), p(all_off), n, p(out), stream))

    do_rank(bits, 0)                                   # (rank, src and out_off of the selection stay as the single stages need them)
    select_alone(True)
    prefix(nsel)
    calls = {"copy": lambda: copy_to.copy_(dev), "fill_all": fill_all, "rank": lambda: do_rank(bits, 0), "items_select": lambda: select_alone(True),
             "corpus_select": lambda: select_alone(False), "fill": lambda: do_fill(nsel), "items_route": lambda: route(bits, True),
             "corpus_route": lambda: route(bits, False), "torch_route": lambda: torch_route(bits),
             "contains_corpus": lambda: r.contains_corpus_bits(corpus, out=zeros), "contains_items": lambda: r.contains_items_bits(items, out=zeros)}
    calls.update(one)
    for call in calls.values():
        call()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(launches):
        for k, call in calls.items():                       # alternating: every call has the others right beside it
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); call(); b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in ms.items()}
    line = {"config": kind, "entry": "filter", "bytes": nbytes, "lines": n, "stripe": corpus.stripe, "selected": nsel, "selected_bytes": total, "launches": launches}
    for k in calls:
        line[k + "_ms"] = round(med[k], 4)
        line[k + "_spread_ms"] = round(spread[k], 4)
    line["copy_GB/s"] = round(nbytes / med["copy"] / 1e6, 1)
    line["fill_all_GB/s"] = round(nbytes / med["fill_all"] / 1e6, 1)
    line["fill_all_share_of_copy"] = round(med["copy"] / med["fill_all"], 4)
    line["fill_GB/s"] = round(total / med["fill"] / 1e6, 1)
    beats = lambda x, y: bool(med[y] - med[x] > spread[x] + spread[y])       # beyond the sum of the two spreads
    for x, y in (("corpus_select", "items_select"), ("corpus_route", "items_route"), ("corpus_route", "torch_route"), ("items_route", "torch_route"),
                 ("one_call_corpus", "one_call_items"), ("one_call_items", "one_call_extents")):
        line[x + "_over_" + y] = round(med[x] / med[y], 4)
        line[x + "_beats_" + y], line[y + "_beats_" + x] = beats(x, y), beats(y, x)
    print(json.dumps(line), flush=True)


def pieces_child(rr, r, kind, dev, off, launches, skew):
    """copy, replace's fill at rep_len 0, pieces fill on GAPS and on MATCHES, pieces sizes and both one-call forms, alternating."""
    import ctypes as C
    import torch
    L, s, nbytes = rr._L, rr._stream_ptr(None), int(dev.numel())
    ptr = lambda t: C.c_void_p(t.data_ptr())
    rounds = 3
    if skew:                                   # the first SKEW_ITEMS items: the lines up to the first line start at or behind k * SKEW_ITEM_BYTES
        cuts = torch.searchsorted(off, torch.arange(1, SKEW_ITEMS + 1, device="cuda") * SKEW_ITEM_BYTES)
        assert int(cuts[-1]) < off.numel() - 1, "the text is too short for the skewed batch"
        off = torch.cat([off[:1], off[cuts], off[int(cuts[-1]) + 1:]]).contiguous()
        rounds, launches = 2, 2
    n = off.numel() - 1
    first, start, end = r.search_all_longest_extents_fused(dev, off, trim=1)
    nmatches = int(start.numel())
    if not nmatches:
        start = end = torch.zeros(1, dtype=torch.int32, device="cuda")
    copy_to = torch.empty_like(dev)
    # replace at rep_len 0: the baseline of the A/B
    length, pos = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(max(nmatches, 1), dtype=torch.int32, device="cuda")
    rr._check(L.rrx_replace_matches_sizes(0, ptr(off), n, 1, ptr(first), ptr(start), ptr(end), 0, ptr(length), ptr(pos), s))
    out_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(length.to(torch.int64), dim=0, out=out_off[1:])
    rep_out = torch.empty(int(out_off[-1]), dtype=torch.uint8, device="cuda")
    replace_fill = lambda: rr._check(L.rrx_replace_matches_fill(0, ptr(dev), ptr(off), n, 1, ptr(first), ptr(end), ptr(pos), None, 0, ptr(out_off), ptr(rep_out), s))
    # the pieces of both modes
    col = {}
    for mode, name in ((1, "gaps"), (0, "matches")):
        npieces = nmatches + (n if mode else 0)
        list_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        plen, psrc = torch.empty(max(npieces, 1), dtype=torch.int32, device="cuda"), torch.empty(max(npieces, 1), dtype=torch.int64, device="cuda")
        sizes = lambda mode=mode, list_off=list_off, plen=plen, psrc=psrc: rr._check(L.rrx_pieces_sizes(0, ptr(off), n, 1, ptr(first), ptr(start), ptr(end), mode,
                                                                                                         ptr(list_off), ptr(plen), ptr(psrc), s))
        sizes()
        poff = torch.zeros(npieces + 1, dtype=torch.int64, device="cuda")
        torch.cumsum(plen[:npieces].to(torch.int64), dim=0, out=poff[1:])
        out = torch.empty(max(int(poff[-1]), 1), dtype=torch.uint8, device="cuda")
        fill = lambda psrc=psrc, poff=poff, npieces=npieces, out=out: rr._check(L.rrx_pieces_fill(0, ptr(dev), ptr(psrc), ptr(poff), npieces, ptr(out), s))
        one_list, one_poff, one_out = torch.empty_like(list_off), torch.empty_like(poff), torch.empty_like(out)
        npc, tot = C.c_size_t(0), C.c_size_t(0)
        fn = L.rrx_split_longest_extents if mode else L.rrx_extract_all_longest_extents
        one = lambda fn=fn, one_list=one_list, one_poff=one_poff, one_out=one_out, npieces=npieces, total=int(poff[-1]), npc=npc, tot=tot: rr._check(
            fn(r._h, 0, ptr(dev), ptr(off), n, 1, ptr(one_list), ptr(one_poff), npieces, ptr(one_out), total, C.byref(npc), C.byref(tot), s))
        col[name] = dict(npieces=npieces, total=int(poff[-1]), sizes=sizes, fill=fill, one=one, out=out, poff=poff, list_off=list_off, one_list=one_list,
                         one_poff=one_poff, one_out=one_out, npc=npc, tot=tot)
    calls = {"copy": lambda: copy_to.copy_(dev), "replace_fill": replace_fill, "gaps_fill": col["gaps"]["fill"], "matches_fill": col["matches"]["fill"],
             "sizes": col["gaps"]["sizes"], "extract_one_call": col["matches"]["one"], "split_one_call": col["gaps"]["one"]}
    for _ in range(1 if skew else 3):
        for call in calls.values():
            call()
    torch.cuda.synchronize()
    print("# %s%s: %d items, %d matches, warmed up" % (kind, "-skewed" if skew else "", n, nmatches), file=sys.stderr, flush=True)
    total = col["gaps"]["total"]
    assert total == int(out_off[-1]) and torch.equal(col["gaps"]["out"][:total], rep_out), "pieces fill on GAPS and replace's fill at rep_len 0 differ"
    for c in col.values():
        assert (c["npc"].value, c["tot"].value) == (c["npieces"], c["total"]) and torch.equal(c["one_out"], c["out"]) and torch.equal(c["one_poff"], c["poff"]) \
            and torch.equal(c["one_list"], c["list_off"]), "a one-call form and the two passes differ"
    meds = {k: [] for k in calls}
    for _ in range(rounds):
        ms = {k: [] for k in calls}
        for _ in range(launches):
            for k, call in calls.items():                   # alternating: every launch has the others right beside it
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); call(); b.record()
                b.synchronize()
                ms[k].append(a.elapsed_time(b))
        for k in calls:
            meds[k].append(statistics.median(ms[k]))
        print("# a round of %d launches done" % launches, file=sys.stderr, flush=True)
    med = {k: statistics.median(v) for k, v in meds.items()}
    line = {"config": kind + ("-skewed" if skew else ""), "entry": "pieces", "bytes": nbytes, "items": n, "matches": nmatches, "gaps_bytes": total,
            "matches_bytes": col["matches"]["total"], "rounds": rounds, "launches": launches}
    for k in calls:
        line[k + "_ms"] = [round(x, 4) for x in meds[k]]
    gbs = lambda nb, ms: nb / ms / 1e6
    line["copy_GB/s"] = round(gbs(nbytes, med["copy"]), 1)                          # bytes copied (read and written once each)
    for k, nb in (("replace_fill", total), ("gaps_fill", total), ("matches_fill", col["matches"]["total"])):
        line[k + "_GB/s"] = round(gbs(nb, med[k]), 1)                               # bytes of the column written
        line[k + "_share_of_copy"] = round(gbs(nb, med[k]) / gbs(nbytes, med["copy"]), 4)
    line["gaps_fill_over_replace_fill"] = round(med["gaps_fill"] / med["replace_fill"], 4)
    line["baseline_margin_ms"] = round(max(meds["replace_fill"]) - min(meds["replace_fill"]), 4)
    line["gaps_fill_within_margin"] = med["gaps_fill"] <= max(meds["replace_fill"])
    print(json.dumps(line), flush=True)


def one_call_child(rr, r, kind, dev, off, launches):
    """The five one-call entries on the first ONE_CALL_ITEMS items with exact caps, alternating; host time per call, one JSON line."""
    import ctypes as C
    import time
    import torch
    assert off.numel() > ONE_CALL_ITEMS, "the text is too short for the batch"
    n, off = ONE_CALL_ITEMS, off[:ONE_CALL_ITEMS + 1].contiguous()
    L, s = rr._L, rr._stream_ptr(None)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t.numel() else None
    i64 = lambda k: torch.empty(k, dtype=torch.int64, device="cuda")
    prefix, tot, npc = i64(n + 1), C.c_size_t(0), C.c_size_t(0)
    calls, found = {}, {}
    for name in ONE_CALL_ENTRIES:                   # a call with cap 0 for the sizes, then the closure with the exact caps
        if name.startswith("search_all"):
            fn = getattr(L, "rrx_%s_extents" % name)
            call = lambda cap, st, en, fn=fn: rr._check(fn(r._h, 0, ptr(dev), ptr(off), n, 1, ptr(prefix), ptr(st), ptr(en), cap, C.byref(tot), s))
            call(0, i64(0), i64(0))
            found[name] = tot.value
            st, en = (torch.empty(tot.value, dtype=torch.int32, device="cuda") for _ in range(2))
            calls[name] = lambda call=call, cap=tot.value, st=st, en=en: call(cap, st, en)
        elif name == "replace_all_longest":
            call = lambda cap, out: rr._check(L.rrx_replace_all_longest_extents(r._h, 0, ptr(dev), ptr(off), n, 1, b"#", 1, ptr(prefix), ptr(out), cap,
                                                                                C.byref(tot), s))
            call(0, i64(0))
            found[name] = tot.value
            out = torch.empty(tot.value, dtype=torch.uint8, device="cuda")
            calls[name] = lambda call=call, cap=tot.value, out=out: call(cap, out)
        else:
            fn = getattr(L, "rrx_%s_extents" % name)
            call = lambda pcap, poff, cap, out, fn=fn: rr._check(fn(r._h, 0, ptr(dev), ptr(off), n, 1, ptr(prefix), ptr(poff), pcap, ptr(out), cap, C.byref(npc),
                                                                    C.byref(tot), s))
            call(0, i64(1), 0, i64(0))
            found[name] = [npc.value, tot.value]
            poff, out = i64(npc.value + 1), torch.empty(tot.value, dtype=torch.uint8, device="cuda")
            calls[name] = lambda call=call, pcap=npc.value, poff=poff, cap=tot.value, out=out: call(pcap, poff, cap, out)
    for _ in range(3):
        for call in calls.values():
            call()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(launches):
        for k, call in calls.items():               # alternating: every call of an entry has the others right beside it
            t0 = time.perf_counter()
            call()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    line = {"config": kind, "entry": "one_call", "lib": os.path.relpath(os.environ["RRX_LIB"], ROOT) if "RRX_LIB" in os.environ else "tree", "items": n, "bytes": int(off[-1] - off[0]), "found": found, "ms": {},
            "spread": {}}
    for k, v in ms.items():
        line["ms"][k] = round(statistics.median(v), 4)
        line["spread"][k] = round((max(v) - min(v)) / statistics.median(v), 4)
    print(json.dumps(line), flush=True)


def one_call_main(a):
    """Four children - parent's library, tree's, parent's, tree's - on this tree's Python; per entry the margin of the other modes."""
    old_lib = os.path.join(a.old, "roaringregex_amd", "librrx.so")
    assert os.path.exists(old_lib), "build the parent commit under %s first" % a.old
    kind, pkey, nbytes = ONE_CALL_TEXT
    runs = {"parent": [], "tree": []}
    for side in ("parent", "tree") * 2:
        env = dict(os.environ)
        env.pop("RRX_LIB", None)
        if side == "parent":
            env["RRX_LIB"] = os.path.abspath(old_lib)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--entry", "one_call", "--launches", str(a.launches), "--child", ROOT, kind, pkey, str(nbytes)],
                           env=env, timeout=300, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode:                       # a fault or a time limit: nothing more is started on the device
            raise SystemExit("child failed with %d: one_call %s" % (p.returncode, side))
        runs[side].append(json.loads(p.stdout.strip().splitlines()[-1]))
    assert all(x["found"] == runs["parent"][0]["found"] for x in runs["parent"] + runs["tree"]), "the two libraries do not find the same"
    assert all(x["lib"] != "tree" for x in runs["parent"]) and all(x["lib"] == "tree" for x in runs["tree"])
    lines = runs["parent"][:1] + runs["tree"][:1] + runs["parent"][1:] + runs["tree"][1:]
    for k in ONE_CALL_ENTRIES:
        pm, tm = [x["ms"][k] for x in runs["parent"]], [x["ms"][k] for x in runs["tree"]]
        margin = max(abs(pm[0] - pm[1]), max(x["spread"][k] * x["ms"][k] for x in runs["parent"]))
        lines.append({"entry": k, "parent_ms": pm, "tree_ms": tm, "margin_ms": round(margin, 4), "within_margin": all(t <= max(pm) + margin for t in tm)})
        print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("tools/probe/item_lanes_rate.py --entry one_call --launches %d: medians of the host time per call [ms] on %d items, the five calls\n"
                "alternating in each of four children (the parent's library through RRX_LIB, the tree's, and again); margin = what the parent\n"
                "differs from itself: the larger of the distance between its two medians and its own spread.\n" % (max(a.launches, 12), ONE_CALL_ITEMS))
        for x in lines:
            f.write(json.dumps(x) + "\n")


def pieces_main(a):
    """One child per text and one for the skewed batch, this tree alone; the lines to a.out as they come."""
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("tools/probe/item_lanes_rate.py --entry pieces --launches %d --scale %g: per call the medians [ms] of three rounds of launches (the\n"
                "skewed batch: two rounds of two), device-event times, the seven calls alternating in one process per text; GB/s = bytes of the\n"
                "column written (the fills) or copied (copy) per second; gaps_fill writes the bytes replace_fill writes: that pair is the A/B,\n"
                "its margin the spread of replace_fill's own medians.\n" % (a.launches, a.scale))
        skewed = ("url-skewed", "U2", SKEW_ITEMS * SKEW_ITEM_BYTES + (256 << 20))
        for kind, pkey, nbytes in CONFIGS + (skewed,):
            n = nbytes if kind.endswith("-skewed") else int(nbytes * a.scale) // 4096 * 4096
            env = dict(os.environ)
            env.pop("RRX_LIB", None)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--entry", "pieces", "--launches", str(a.launches), "--child", ROOT, kind, pkey, str(n)],
                               env=env, timeout=900, stdout=subprocess.PIPE, text=True)
            sys.stdout.write(p.stdout)
            sys.stdout.flush()
            if p.returncode:                   # a fault or a time limit: nothing more is started on the device
                raise SystemExit("child failed with %d: pieces %s" % (p.returncode, kind))
            f.write(p.stdout)
            f.flush()


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


def replace_groups_main(a):
    """One child on the e-mail text (the one text whose pattern has a group put in), this tree alone; the line to a.out."""
    kind, pkey, nbytes = next(c for c in CONFIGS if c[1] in GROUPED)
    n = int(nbytes * a.scale) // 4096 * 4096
    env = dict(os.environ)
    env.pop("RRX_LIB", None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--entry", "replace_groups", "--launches", str(a.launches), "--child", ROOT, kind, pkey, str(n)],
                       env=env, timeout=600, stdout=subprocess.PIPE, text=True)
    sys.stdout.write(p.stdout)
    sys.stdout.flush()
    if p.returncode:                           # a fault or a time limit: nothing more is started on the device
        raise SystemExit("child failed with %d: replace_groups %s" % (p.returncode, kind))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("tools/probe/item_lanes_rate.py --entry replace_groups --launches %d --scale %g: medians of device-event times per call [ms], all\n"
                "calls alternating in one process; pattern %s, literal %r; *_parent_literal = the literal entries, whose code the\n"
                "parent commit has unchanged.\n" % (a.launches, a.scale, GROUPED[pkey], REPLACE_GROUPS_LITERAL.decode()))
        f.write(p.stdout)


def multi_contains_main(a):
    """One child on the keyword-log text, this tree alone; the lines and the break-even K to a.out."""
    kind, pkey, nbytes = next(c for c in CONFIGS if c[0] == "kwlog")
    n = int(nbytes * a.scale) // 4096 * 4096
    env = dict(os.environ)
    env.pop("RRX_LIB", None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--entry", "multi_contains", "--launches", str(a.launches), "--child", ROOT, kind, pkey, str(n)],
                       env=env, timeout=600, stdout=subprocess.PIPE, text=True)
    sys.stdout.write(p.stdout)
    sys.stdout.flush()
    if p.returncode:                           # a fault or a time limit: nothing more is started on the device
        raise SystemExit("child failed with %d: multi_contains %s" % (p.returncode, kind))
    lines = [json.loads(x) for x in p.stdout.strip().splitlines()]
    wins = [x["K"] for x in lines if x["multi_ms"] < x["singles_ms"]]
    summary = {"entry": "multi_contains", "launches": max(a.launches, 12), "scale": a.scale, "K": [x["K"] for x in lines],
               "multi_over_singles": [x["multi_over_singles"] for x in lines], "break_even_K": min(wins) if wins else None}
    print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("tools/probe/item_lanes_rate.py --entry multi_contains --launches %d --scale %g: medians of device-event times per call [ms] on the\n"
                "keyword-log text as items (trim 1), one indexed batch; multi = one rrx_multi_contains_items on K keywords (%s ...), singles = K\n"
                "calls of rrx_contains_items, the two alternating in one process; TB/s = bytes of the column per second of the whole question;\n"
                "break_even_K = the smallest measured K at which the set is the faster of the two (null: none).\n"
                % (max(a.launches, 12), a.scale, ", ".join(MULTI_KEYWORDS[:4])))
        for x in lines + [summary]:
            f.write(json.dumps(x) + "\n")


def multi_contains_corpus_main(a):
    """One child on the keyword-log text, this tree alone; the lines and the break-even K against the single calls to a.out."""
    kind, pkey, nbytes = next(c for c in CONFIGS if c[0] == "kwlog")
    n = int(nbytes * a.scale) // 4096 * 4096
    env = dict(os.environ)
    env.pop("RRX_LIB", None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--entry", "multi_contains_corpus", "--launches", str(a.launches), "--child", ROOT, kind, pkey,
                        str(n)], env=env, timeout=600, stdout=subprocess.PIPE, text=True)
    sys.stdout.write(p.stdout)
    sys.stdout.flush()
    if p.returncode:                           # a fault or a time limit: nothing more is started on the device
        raise SystemExit("child failed with %d: multi_contains_corpus %s" % (p.returncode, kind))
    lines = [json.loads(x) for x in p.stdout.strip().splitlines()]
    wins = [x["K"] for x in lines if x["corpus_beats_singles"]]
    summary = {"entry": "multi_contains_corpus", "launches": max(a.launches, 12), "scale": a.scale, "K": [x["K"] for x in lines],
               "corpus_over_items": [x["corpus_over_items"] for x in lines], "corpus_over_singles": [x["corpus_over_singles"] for x in lines],
               "corpus_beats_items": [x["corpus_beats_items"] for x in lines], "items_beats_corpus": [x["items_beats_corpus"] for x in lines],
               "break_even_K": min(wins) if wins else None}
    print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("tools/probe/item_lanes_rate.py --entry multi_contains_corpus --launches %d --scale %g: medians of device-event times per call [ms] on the\n"
                "keyword-log text; corpus = one rrx_multi_contains_corpus on K keywords (%s ...) over the text as an rrx_corpus, singles = K calls\n"
                "of rrx_contains_corpus on it, items = one rrx_multi_contains_items on an indexed batch over the same lines (trim 1), the three\n"
                "alternating in one process; spread = (max - min) / median, spread_ms = max - min; TB/s = bytes of the text per second of the whole\n"
                "question; x_beats_y = the medians differ by more than the sum of the two spreads [ms]; break_even_K = the smallest measured K\n"
                "at which corpus beats singles (null: none).\n"
                % (max(a.launches, 12), a.scale, ", ".join(MULTI_KEYWORDS[:4])))
        for x in lines + [summary]:
            f.write(json.dumps(x) + "\n")


def search_longest_corpus_main(a):
    """One child per text - the keyword log and the e-mail text -, this tree alone; the lines to a.out."""
    lines = []
    for kind, pkey, nbytes in (c for c in CONFIGS if c[0] in ("kwlog", "email")):
        n = int(nbytes * a.scale) // 4096 * 4096
        env = dict(os.environ)
        env.pop("RRX_LIB", None)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--entry", "search_longest_corpus", "--launches", str(a.launches), "--child", ROOT, kind,
                            pkey, str(n)], env=env, timeout=600, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode:                       # a fault or a time limit: nothing more is started on the device
            raise SystemExit("child failed with %d: search_longest_corpus %s" % (p.returncode, kind))
        lines.append(json.loads(p.stdout.strip().splitlines()[-1]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("tools/probe/item_lanes_rate.py --entry search_longest_corpus --launches %d --scale %g: medians of device-event times per call [ms];\n"
                "corpus = rrx_search_longest_corpus on the text as an rrx_corpus, items = rrx_search_longest_items on an indexed batch over the same\n"
                "lines (trim 1; its offsets array is built beforehand and not timed), first = rrx_search_corpus on the same corpus - another question,\n"
                "the yardstick for what two passes cost; the three alternating in one process, corpus == items word for word before timing; spread =\n"
                "(max - min) / median, spread_ms = max - min; TB/s = bytes of the text per second; x_beats_y = the medians differ by more than the\n"
                "sum of the two spreads [ms].\n" % (max(a.launches, 12), a.scale))
        for x in lines:
            f.write(json.dumps(x) + "\n")


def filter_main(a):
    """One child per text - the keyword log and the e-mail text -, this tree alone (the parent has no such entry); the lines to a.out."""
    lines = []
    for kind, pkey, nbytes in (c for c in CONFIGS if c[0] in ("kwlog", "email")):
        n = int(nbytes * a.scale) // 4096 * 4096
        env = dict(os.environ)
        env.pop("RRX_LIB", None)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--entry", "filter", "--launches", str(a.launches), "--child", ROOT, kind, pkey, str(n)],
                           env=env, timeout=600, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode:                       # a fault or a time limit: nothing more is started on the device
            raise SystemExit("child failed with %d: filter %s" % (p.returncode, kind))
        lines.append(json.loads(p.stdout.strip().splitlines()[-1]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("tools/probe/item_lanes_rate.py --entry filter --launches %d --scale %g: medians of device-event times per call [ms], all calls\n"
                "alternating in one process per text; x_spread_ms = max - min.  copy = a device-to-device copy of the column; fill_all =\n"
                "rrx_pieces_fill of every line with its newline (the invert of an all-zero bitmap: the output is the text).  On the pattern's\n"
                "contains bitmap: rank = rrx_bitmap_rank, items_select = rrx_filter_sizes (trim 1), corpus_select = rrx_filter_corpus_sizes,\n"
                "fill = rrx_pieces_fill of the selected lines; items_route / corpus_route = rank, the count read back, select, torch.cumsum, the\n"
                "size read back, fill; torch_route = what a caller did before: rrx_bitmap_to_bytes, torch.nonzero, indexing the offsets, cumsum,\n"
                "the size read back, rrx_pieces_fill (it needs the offsets array, which a corpus does not have); contains_* = the bitmap alone;\n"
                "one_call_* = rrx_filter_contains_extents / _items / _corpus, contains included.  All routes and one-call forms gave the same\n"
                "column before timing.  GB/s = bytes written per second.  x_beats_y = the medians differ by more than the sum of the two\n"
                "spreads [ms].\n" % (max(a.launches, 12), a.scale))
        for x in lines:
            f.write(json.dumps(x) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entry", choices=ENTRIES, required=True)
    ap.add_argument("--old", default=os.path.join(ROOT, ".oldtree"))
    ap.add_argument("--launches", type=int, default=15)
    ap.add_argument("--scale", type=float, default=1.0, help="corpus sizes times this (a quick run)")
    ap.add_argument("--out", default=None, help="--entry replace / pieces: where the lines and the summary go (default: profiles/<entry>_items_rate.txt)")
    ap.add_argument("--child", nargs=4, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        tree, kind, pkey, nbytes = a.child
        return child(tree, a.entry, kind, pkey, int(nbytes), max(a.launches, 12))
    if a.out is None:
        stem = {"replace_groups": "replace_template_items", "multi_contains_corpus": "multi_contains_corpus",
                "search_longest_corpus": "search_longest_corpus", "filter": "filter"}.get(a.entry, a.entry + "_items")
        a.out = os.path.join(ROOT, "profiles", stem + "_rate.txt")
    if a.entry == "replace":
        return replace_main(a)
    if a.entry == "pieces":
        return pieces_main(a)
    if a.entry == "one_call":
        return one_call_main(a)
    if a.entry == "replace_groups":
        return replace_groups_main(a)
    if a.entry == "multi_contains":
        return multi_contains_main(a)
    if a.entry == "multi_contains_corpus":
        return multi_contains_corpus_main(a)
    if a.entry == "search_longest_corpus":
        return search_longest_corpus_main(a)
    if a.entry == "filter":
        return filter_main(a)
    assert os.path.exists(os.path.join(a.old, "roaringregex_amd", "librrx.so")), "build the parent commit under %s first" % a.old
    # a parent that has the entry runs the entry itself: the yardsticks are for the commit that added it
    yardstick = a.entry in YARDSTICK and NEWER[a.entry] not in open(os.path.join(a.old, "roaringregex_amd", "__init__.py")).read()
    for kind, pkey, nbytes in CONFIGS:
        n = int(nbytes * a.scale) // 4096 * 4096
        runs = {"parent": [], "tree": []}
        for side, tree in (("parent", a.old), ("tree", ROOT)) * 2:
            env = dict(os.environ)
            env.pop("RRX_LIB", None)
            entry = YARDSTICK[a.entry] if side == "parent" and yardstick else a.entry
            key = pkey + "+group" if a.entry == "extract_group" else pkey
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--entry", entry, "--launches", str(a.launches), "--child", tree, kind, key, str(n)],
                               env=env, timeout=600, stdout=subprocess.PIPE, text=True)
            sys.stdout.write(p.stdout)
            sys.stdout.flush()
            if p.returncode:                   # a fault or a time limit: nothing more is started on the device
                raise SystemExit("child failed with %d: %s %s %s" % (p.returncode, tree, entry, kind))
            runs[side].append(json.loads(p.stdout.strip().splitlines()[-1]))
        if yardstick and a.entry in SAME_ITEMS:
            assert len({x["found"] for x in runs["parent"] + runs["tree"]}) == 1, "the two sides do not find a match in the same items"
            parent_ms, tree_ms = statistics.median(x["ms"] for x in runs["parent"]), statistics.median(x["ms"] for x in runs["tree"])
            print("# parent side: %s, tree side: %s, the same pattern and items; tree / parent = %.3f (%.3f against %.3f TB/s)"
                  % (YARDSTICK[a.entry], a.entry, tree_ms / parent_ms, runs["tree"][0]["bytes"] / tree_ms / 1e9, runs["parent"][0]["bytes"] / parent_ms / 1e9))
        elif yardstick:
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
