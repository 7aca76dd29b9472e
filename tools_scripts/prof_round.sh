#!/bin/bash
# rocprofv3 --kernel-trace --stats of the bench workload (--full without the
# PMC child, the CPU legs and the end-to-end worker): the per-kernel averages
# the bench line's roofline is checked against.  Results go to $OUT (default
# ./out).   tools_scripts/prof_round.sh TAG
set -o pipefail
export TMPDIR=/tmp
R=$PWD
OUT=${OUT:-$R/out}
mkdir -p $OUT
cd /tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT/prof_${1:-round} --output-format csv \
  -- python3 $R/bench.py --full --no-pmc --no-cpu --no-full-build > $OUT/prof_${1:-round}_bench.json 2> $OUT/prof_${1:-round}_bench.err \
  || { echo "rocprof failed"; tail -20 $OUT/prof_${1:-round}_bench.err; exit 1; }
echo prof-done
