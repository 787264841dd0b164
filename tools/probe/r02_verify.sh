#!/bin/bash
# full verification on the GPU box: the -m gpu suite, smoke(), two fuzz runs (small corpora with the cooperative engines; 4 MiB corpora)
PROBE_OUT=${PROBE_OUT:-probe_out}         # results, relative to the repository root
R=$GRAFT_REPO_ROOT; [ -z "$R" ] && R=/root/repo
cd $R; mkdir -p $PROBE_OUT
TAG=${1:-verify}
( time timeout -k 10 1000 python -m pytest tests -m gpu -x -q ) > $PROBE_OUT/${TAG}_tests.log 2>&1; echo "tests rc=$?" >> $PROBE_OUT/${TAG}_tests.log; tail -8 $PROBE_OUT/${TAG}_tests.log
python -c "import __graft_entry__ as g; g.smoke()" > $PROBE_OUT/${TAG}_smoke.log 2>&1; echo "smoke rc=$?" >> $PROBE_OUT/${TAG}_smoke.log; tail -2 $PROBE_OUT/${TAG}_smoke.log
timeout -k 10 400 python tools/fuzz/gpu_fuzz.py 11 120 > $PROBE_OUT/${TAG}_fuzz_small.txt 2>&1; tail -2 $PROBE_OUT/${TAG}_fuzz_small.txt
timeout -k 10 500 python tools/fuzz/gpu_fuzz.py 12 40 4194304 > $PROBE_OUT/${TAG}_fuzz_big.txt 2>&1; tail -2 $PROBE_OUT/${TAG}_fuzz_big.txt
