"""What rrx_search_longest_string / rrx_contains_string cost on ONE long device-resident string, against rrx_match_string on the
same bytes (what the chunk machinery costs for the END state alone) and against the only route there was before, one item of
rrx_search_longest_extents (a single lane, twice over the text); and where the chunk route and the one-item route cross on short
strings.  Writes profiles/search_longest_string_rate.txt (--out).

    python tools/probe/search_string_rate.py                 rates and crossing, on a device
    python tools/probe/search_string_rate.py --resources     appends the compiler's report on the two new kernels (no device)

Times are host clocks around calls that end in a device synchronise (the entries are synchronous), after a warm-up call, medians
of repeated calls, the compared routes alternating inside one process.  The crossing is measured in a child process on
roaringregex_amd/librrx_search_from256.so (make -C roaringregex_amd/csrc search-from256: the same library with the hand-over
threshold at 256 bytes, loaded through RRX_LIB), so that the chunk route is timed below the compiled threshold too."""
import argparse
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..", "..")
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

KW = "k(123|456|789|1000)"
FROM256 = os.path.join(ROOT, "roaringregex_amd", "librrx_search_from256.so")
GIB = 1 << 30


def W5():
    return "c((a|b){5})*d"


def medians(routes, reps):
    """routes: name -> call.  One warm-up each, then `reps` rounds in which the routes take turns.  -> name -> median seconds"""
    import torch
    for f in routes.values():
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in routes}
    for _ in range(reps):
        for k, f in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    return {k: statistics.median(v) for k, v in times.items()}


def texts(n):
    """name -> (pattern, n bytes).  The W(5) text is one match from its first byte to its last: every chunk flagged, both passes
    over the whole string."""
    import numpy as np
    import synth
    yield "url text, U2", __import__("patterns").U2, synth.corpus("url", 1, n, threads=16)
    yield "keyword-log text, " + KW, KW, synth.corpus("kwlog", 1, n, threads=16)
    nab = 5 * ((n - 2) // 5)
    w = np.full(n, ord("z"), dtype=np.uint8)
    w[0] = ord("c")
    w[1:1 + nab] = ord("a") + np.random.default_rng(1).integers(0, 2, size=nab, dtype=np.uint8)
    w[1 + nab] = ord("d")
    yield "W(5) text, one match over the whole string", W5(), w


def one_item(r, dev):
    import torch
    off = torch.tensor([0, dev.numel()], dtype=torch.int64, device="cuda")
    return lambda: r.search_longest_extents(dev, off)


def rates(out):
    import torch
    import roaringregex_amd as rr
    out("device: %s; library: %s" % (torch.cuda.get_device_name(0), os.path.basename(rr._SO)))
    out("")
    out("== 1 GiB strings: the new entries against rrx_match_string on the same bytes (median of 5 calls, ms; GB/s of the string's bytes)")
    for name, pat, text in texts(GIB):
        r = rr.RRegex(pat)
        dev = torch.from_numpy(text).cuda()
        span = r.search_longest_string(dev)
        t = medians({"search": lambda: r.search_longest_string(dev), "contains": lambda: r.contains_string(dev),
                     "match": lambda: r.match_string(dev)}, 5)
        out("%s: match [%d, %d)" % (name, span[0], span[1]))
        for k in ("search", "contains", "match"):
            out("    %-28s %9.3f ms  %8.1f GB/s" % ({"search": "rrx_search_longest_string", "contains": "rrx_contains_string",
                                                      "match": "rrx_match_string"}[k], t[k] * 1e3, GIB / t[k] / 1e9))
        out("    search / match = %.2f, contains / match = %.2f" % (t["search"] / t["match"], t["contains"] / t["match"]))
        out("  the one-item route (rrx_search_longest_extents, one lane) against the chunk route on a prefix (median of 3 calls):")
        for mib in (1, 4, 16):
            n = mib << 20
            part = text[:n].copy()
            if pat == W5():                                   # (a prefix of the match is no match: end it)
                part[1 + 5 * ((n - 2) // 5)] = ord("d")
            d = torch.from_numpy(part).cuda()
            t = medians({"chunks": lambda: r.search_longest_string(d), "one item": one_item(r, d)}, 3)
            out("    %3d MiB: one item %10.3f ms = %6.1f ns per byte;  chunks %8.3f ms;  one item / chunks = %.0f" %
                (mib, t["one item"] * 1e3, t["one item"] / n * 1e9, t["chunks"] * 1e3, t["one item"] / t["chunks"]))
            del d
        del dev, text
        out("")


def crossing(out):
    """(in the child, on the from-256 library)"""
    import torch
    import synth
    import roaringregex_amd as rr
    from patterns import U2
    out("== the crossing on url text, U2: chunk route (library with the threshold at 256: %s) against the one-item route,"
        % os.path.basename(rr._SO))
    out("   median of 21 calls, us")
    text = synth.corpus("url", 1, 1 << 20, threads=16)
    r = rr.RRegex(U2)
    first = None
    for n in (256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536):
        d = torch.from_numpy(text[:n].copy()).cuda()
        t = medians({"chunks": lambda: r.search_longest_string(d), "one item": one_item(r, d)}, 21)
        wins = t["chunks"] < t["one item"]
        if wins and first is None:
            first = n
        if not wins:
            first = None
        out("    %6d B: chunks %8.1f us   one item %8.1f us   %s" % (n, t["chunks"] * 1e6, t["one item"] * 1e6, "chunks win" if wins else "one item wins"))
    out("   the chunk route wins from %s on" % ("%d bytes" % first if first else "no length measured here"))
    out("")


def resources(out):
    csrc = os.path.join(ROOT, "roaringregex_amd", "csrc")
    rep = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c",
                          "kernels_long_search.hip", "-o", os.devnull], cwd=csrc, stderr=subprocess.PIPE, text=True, check=True).stderr
    out("== the compiler's report (-Rpass-analysis=kernel-resource-usage) on the two new kernels; their LDS is dynamic: the table,")
    out("   states x 129 x 2 bytes (at most 65532), for long_extreme_kernel; a group's maps, 128 x states x 2 bytes, and 512 bytes of")
    out("   entries for long_entries_kernel")
    name, keep = None, ("VGPRs:", "SGPRs:", "ScratchSize", "Occupancy", "LDS Size")
    for line in rep.splitlines():
        text = line.split("remark:", 1)[-1].strip().replace(" [-Rpass-analysis=kernel-resource-usage]", "")
        if text.startswith("Function Name:"):
            name = text if ("long_entries_kernel" in text or "long_extreme_kernel" in text) else None
            if name:
                out("    " + name.replace("Function Name: ", "") + ("  (backward)" if "ILb1E" in name else "  (forward)" if "ILb0E" in name else ""))
        elif name and any(k in text for k in keep):
            out("        " + text)
    out("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_longest_string_rate.txt"))
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--crossing-child", action="store_true")
    a = ap.parse_args()
    with open(a.out, "a" if (a.resources or a.crossing_child) else "w") as f:
        def out(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        if a.resources:
            return resources(out)
        if a.crossing_child:
            return crossing(out)
        out("tools/probe/search_string_rate.py")
        rates(out)
    if os.path.exists(FROM256):
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--out", a.out, "--crossing-child"], env=dict(os.environ, RRX_LIB=FROM256))
    else:
        with open(a.out, "a") as f:
            f.write("== the crossing: not measured (no librrx_search_from256.so: make -C roaringregex_amd/csrc search-from256)\n")


if __name__ == "__main__":
    main()
