#!/bin/bash
# One GPU call on the current tree: the full -m gpu suite, smoke(), the
# bench's --full line (with the end-to-end worker build), and a
# rocprofv3 kernel-trace --stats of the bench workload.  Logs and results go
# to $OUT (default ./out).
#   tools_scripts/gpu_round.sh TAG [skip-tests] [skip-prof]
set -o pipefail
TAG=${1:-round}
R=$PWD
OUT=${OUT:-$R/out}
mkdir -p $OUT
export TMPDIR=/tmp
if [ "$2" != "skip-tests" ]; then
  timeout -k 10 1000 python -u -m pytest tests -m gpu -x -v --timeout 600 --timeout-method thread --durations=20 \
      > $OUT/${TAG}_gputest.log 2>&1 || { echo "GPU TESTS FAILED"; tail -60 $OUT/${TAG}_gputest.log; exit 1; }
  tail -3 $OUT/${TAG}_gputest.log
fi
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > $OUT/${TAG}_smoke.log 2>&1 \
    || { echo "smoke failed"; tail -20 $OUT/${TAG}_smoke.log; exit 1; }
tail -1 $OUT/${TAG}_smoke.log
timeout -k 10 700 python bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err \
    || { echo "bench failed"; tail -20 $OUT/${TAG}_bench.err; exit 1; }
cat $OUT/${TAG}_bench.json
if [ "$3" != "skip-prof" ]; then
  cd /tmp
  timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG --output-format csv \
      -- python3 $R/bench.py --full --no-pmc --no-cpu --no-full-build > $OUT/prof_${TAG}_bench.json 2> $OUT/prof_${TAG}_bench.err \
      || { echo "rocprof failed"; tail -20 $OUT/prof_${TAG}_bench.err; exit 1; }
  echo prof-done
fi
