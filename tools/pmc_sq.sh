R=$(cd "$(dirname "$0")/.." && pwd); OUT=${OUT:-$R/prof_out}; mkdir -p "$OUT"; cd /tmp; export TMPDIR=/tmp
rm -rf $OUT/pmc_lds $OUT/pmc_sqb
timeout 200 rocprofv3 --pmc SQ_INSTS_LDS SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_LDS_ADDR_CONFLICT SQ_WAVE_CYCLES SQ_BUSY_CYCLES --kernel-trace --output-format csv -d $OUT/pmc_lds -o b -- python $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > $OUT/pmc_lds.log 2>&1
timeout 200 rocprofv3 --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY --kernel-trace --output-format csv -d $OUT/pmc_sqb -o b -- python $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > $OUT/pmc_sqb.log 2>&1
ls $OUT/pmc_lds $OUT/pmc_sqb; tail -2 $OUT/pmc_lds.log | cut -c1-200
