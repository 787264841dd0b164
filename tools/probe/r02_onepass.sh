#!/bin/bash
PROBE_OUT=${PROBE_OUT:-probe_out}         # results, relative to the repository root
R=$GRAFT_REPO_ROOT; [ -z "$R" ] && R=/root/repo
cd $R; mkdir -p $PROBE_OUT
timeout -k 10 600 python -m pytest tests -m gpu -x -q -k "one_shot or kat_batch or golden" > $PROBE_OUT/op_tests.log 2>&1; echo "tests rc=$?" >> $PROBE_OUT/op_tests.log; tail -25 $PROBE_OUT/op_tests.log
bash tools/probe/r02_run.sh op notests "auto" "url email arepeat kwlines kwlog"
