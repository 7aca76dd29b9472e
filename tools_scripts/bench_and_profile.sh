# One GPU call: the bench's --full line (with its PMC child passes and CPU
# baseline), then a rocprofv3 kernel-trace of the same workload for profiles/.
# Results go to $OUT (default ./out of the repository).
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/out}
TAG=${1:-r01}
mkdir -p $OUT
timeout -k 10 600 python3 -u $R/bench.py --full > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err
echo bench-done
cat $OUT/bench_$TAG.json
cd /tmp && export TMPDIR=/tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG --output-format csv -- python3 $R/bench.py --full --no-pmc --no-cpu > $OUT/prof_${TAG}_bench.json 2> $OUT/prof_${TAG}_bench.err
echo prof-done
