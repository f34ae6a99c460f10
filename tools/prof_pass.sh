# usage (on a machine with the GPU): bash tools/prof_pass.sh TAG "COUNTER COUNTER ..." [bench args]   -> $OUT/pmc_TAG/ (OUT: prof_out/)
# one rocprofv3 counter pass of bench.py --full (kernel trace + the given PMC counters, csv)
R=$(cd "$(dirname "$0")/.." && pwd); OUT=${OUT:-$R/prof_out}; mkdir -p "$OUT"; TAG=$1; CTRS=$2; shift 2
cd /tmp; export TMPDIR=/tmp
rm -rf $OUT/pmc_$TAG
timeout 300 rocprofv3 --pmc $CTRS --kernel-trace --output-format csv -d $OUT/pmc_$TAG -o b -- python $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-verify --no-ntt --no-concurrent --no-other-configs "$@" > $OUT/pmc_$TAG.log 2>&1
ls $OUT/pmc_$TAG | head -3
