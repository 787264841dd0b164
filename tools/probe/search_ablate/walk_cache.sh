#!/bin/bash
# How much of the walks' time is text that has left the caches?  The first-match kernel rebuilt with the walks reading their text from the
# FIRST 4 KiB of the corpus (always in the L1/L2: the results are wrong, the turn counts those of the same kind of text), against the
# shipping kernel and against "no walks".  usage: walk_cache.sh <workload> <bytes>
# A variant whose sed script no longer changes the source stops the run: it would time the unmodified kernel under the variant's name.
R=$(cd "$(dirname "$0")/../../.." && pwd)
W=${1:-email}; N=${2:-1073741824}
S=${ABLATE_DIR:-/tmp/ablate}; rm -rf $S; mkdir -p $S; cp -r $R/roaringregex_amd $R/include $R/tools $R/bench.py $R/tests $S/ 2>/dev/null
cd $S/roaringregex_amd/csrc
SRC=kernels_search.hip
cp $SRC $SRC.orig
variant() {  # name, sed scripts (each must change the source)
  local name=$1; shift
  cp $SRC.orig $SRC
  for script in "$@"; do
    cp $SRC $SRC.before; sed -i "$script" $SRC
    if cmp -s $SRC $SRC.before; then echo "variant '$name': an edit matched nothing in $SRC - re-anchor it: $script" >&2; exit 1; fi
  done
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC -Wno-unused-parameter --offload-arch=gfx950 -c $SRC -o build/$SRC.o 2> /tmp/ablate_cc.log || { tail -5 /tmp/ablate_cc.log; exit 1; }
  [ -n "$ABLATE_COMPILE_ONLY" ] && { echo "$name: compiles"; return; }
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -shared -o ../librrx.so build/*.o || exit 1
  echo -n "$name: "; (cd $S && timeout -k 10 120 python3 tools/probe/search_run.py $W $N 5) || exit 1
}
# text_word: the walks read the first 4 KiB
C='s|^    auto text_word = \[&\](uint32_t at) -> uint32_t { return \*reinterpret_cast<const uint32_t \*>(cbase + at); };.*$|    auto text_word = [\&](uint32_t at) -> uint32_t { return *reinterpret_cast<const uint32_t *>(bytes + (at \& 0xffcu)); };|'
# drain: the jobs are dropped
D='s|^        const uint32_t count = fill;$|        const uint32_t count = 0; if (nbytes) { fill = 0; return; }|'
variant "all phases                      "
variant "walks read cached text (wrong!) " "$C"
variant "no walks                        " "$D"
