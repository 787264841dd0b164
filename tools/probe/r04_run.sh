#!/bin/bash
# round-4 measurement set.  usage: r04_run.sh <tag> [tests|notests] [all|default]
R=$GRAFT_REPO_ROOT; [ -z "$R" ] && R=/root/repo
O=${PROBE_OUT:-probe_out}                 # results, relative to the repository root
cd $R; mkdir -p $O
TAG=${1:-r04}; DO_TESTS=${2:-tests}; WHAT=${3:-all}
if [ "$DO_TESTS" = tests ]; then
  timeout -k 10 1100 python -m pytest tests -m gpu -x -q > $O/${TAG}_tests.log 2>&1 || { tail -40 $O/${TAG}_tests.log; exit 1; }
  tail -3 $O/${TAG}_tests.log
fi
timeout -k 10 400 python bench.py --full > $O/${TAG}_default.json 2> $O/${TAG}_default.err || { tail -5 $O/${TAG}_default.err; exit 1; }
python -c "import json;d=json.loads(open('$O/${TAG}_default.json').read().strip().splitlines()[-1]);print('url',d['value'],d['roofline']['frac'],d['roofline']['kernel_ms_avg'],d['cold'])"
if [ "$WHAT" = all ]; then
  : > $O/${TAG}_all.txt
  for w in email arepeat kwlines kwlog; do
    timeout -k 10 300 python bench.py --full --workload $w --no-cpu-baseline >> $O/${TAG}_all.txt 2>> $O/${TAG}_all.err || { tail -5 $O/${TAG}_all.err; exit 1; }
  done
  python - <<PY
import json
for l in open('$O/${TAG}_all.txt'):
    l=l.strip()
    if l.startswith('{'):
        d=json.loads(l); print(d['config']['workload'], d['value'], d['roofline']['frac'], d['roofline']['kernel_ms_avg'], d.get('cold'))
PY
fi
