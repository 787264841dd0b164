#!/bin/bash
PROBE_OUT=${PROBE_OUT:-probe_out}         # results, relative to the repository root
R=$GRAFT_REPO_ROOT; [ -z "$R" ] && R=/root/repo
cd $R; mkdir -p $PROBE_OUT
TAG=${1:-srch}
timeout -k 10 600 python -m pytest tests -m gpu -x -q -k "search" > $PROBE_OUT/${TAG}_tests.log 2>&1; echo "tests rc=$?" >> $PROBE_OUT/${TAG}_tests.log; tail -25 $PROBE_OUT/${TAG}_tests.log
: > $PROBE_OUT/${TAG}_bench.txt
for W in url email kwlog; do
timeout -k 10 300 python bench.py --steps 5 --warmup 1 --no-cpu-baseline --workload $W --search 2>$PROBE_OUT/${TAG}_bench.err | python -c "import sys,json; d=json.loads(sys.stdin.read()); print('$W', d['config']['engine'], d['value'], d['search'])" >> $PROBE_OUT/${TAG}_bench.txt
tail -1 $PROBE_OUT/${TAG}_bench.txt
done
