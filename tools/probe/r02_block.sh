#!/bin/bash
PROBE_OUT=${PROBE_OUT:-probe_out}         # results, relative to the repository root
R=$GRAFT_REPO_ROOT; [ -z "$R" ] && R=/root/repo
cd $R; mkdir -p $PROBE_OUT
timeout -k 10 1000 python -m pytest tests -m gpu -x -q > $PROBE_OUT/blk_tests.log 2>&1; echo "tests rc=$?" >> $PROBE_OUT/blk_tests.log; tail -12 $PROBE_OUT/blk_tests.log
bash tools/probe/prof.sh r02_group_nondet600 --workload nondet600 > /dev/null 2>&1
cat $PROBE_OUT/prof_r02_group_nondet600/summary.txt | head -30
