#!/bin/bash
PROBE_OUT=${PROBE_OUT:-probe_out}         # results, relative to the repository root
R=$GRAFT_REPO_ROOT; [ -z "$R" ] && R=/root/repo
cd $R; mkdir -p $PROBE_OUT
timeout -k 10 900 python -m pytest tests -m gpu -x -q > $PROBE_OUT/nfa3_tests.log 2>&1; echo "tests rc=$?" >> $PROBE_OUT/nfa3_tests.log; tail -12 $PROBE_OUT/nfa3_tests.log
bash tools/probe/r02_run.sh nfa3 notests "nfa" "url email arepeat kwlines kwlog nondet"
bash tools/probe/prof.sh r02_nfa_url --workload url --engine nfa > /dev/null 2>&1
bash tools/probe/prof.sh r02_nfa_arepeat --workload arepeat --engine nfa > /dev/null 2>&1
bash tools/probe/prof.sh r02_nfa_nondet --workload nondet --engine nfa > /dev/null 2>&1
ls $PROBE_OUT/prof_r02_nfa_url/ | head
