"""Times the four modes of the stripe-wise search kernel apart: modes.py <workload> <bytes> [repetitions, default 3: one number, or four for first,count,fill,one-call]"""
import os, sys
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", "..", ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import numpy as np, torch
import roaringregex_amd as rr, synth, bench
workload, nbytes = sys.argv[1], int(sys.argv[2])
REPS = [int(x) for x in (sys.argv[3] if len(sys.argv) > 3 else "3").split(",")]
R_FIRST, R_COUNT, R_FILL, R_ALL = REPS * 4 if len(REPS) == 1 else REPS
kind, pkey, _, _ = bench.WORKLOADS[workload]
host = np.empty(nbytes, dtype=np.uint8); synth.fill(kind, 2, host, threads=16)
dev = torch.from_numpy(host).cuda()
corpus = rr.Corpus(dev)
r = rr.RRegex(bench.patterns()[pkey])
def timed(f, reps):
    f(); torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps): out = f()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, out
import ctypes as C
L, n = rr._L, corpus.num_lines
count = torch.zeros(n, dtype=torch.int32, device="cuda")
def do_count():
    rr._check(L.rrx_search_all_count(r._h, corpus._h, C.c_void_p(count.data_ptr()), rr._stream_ptr(None)))
t_first, _ = timed(lambda: r.search_corpus(corpus), R_FIRST)
t_count, _ = timed(do_count, R_COUNT)
inclusive = torch.cumsum(count, dim=0, dtype=torch.int64)
first = (inclusive - count).contiguous()
total = int(inclusive[-1].item())
slots = max(total, 1)     # (a workload without a match: the entries refuse a null pointer)
start = torch.empty(slots, dtype=torch.int32, device="cuda"); end = torch.empty(slots, dtype=torch.int32, device="cuda")
def do_fill():
    rr._check(L.rrx_search_all_fill(r._h, corpus._h, C.c_void_p(first.data_ptr()), C.c_void_p(start.data_ptr()), C.c_void_p(end.data_ptr()), rr._stream_ptr(None)))
t_fill, _ = timed(do_fill, R_FILL)
t_all, _ = timed(lambda: r.search_all_fused(corpus, cap=slots), R_ALL)
print("%s %d MiB: first %.3f ms  count %.3f  fill %.3f  one call %.3f  (lines %d, matches %d)" % (workload, nbytes >> 20, t_first, t_count, t_fill, t_all, n, total))
