#!/bin/bash
# rocprofv3 kernel stats + HBM PMC counters (separate passes) of the bench command
# usage: gpurun -- 'bash tools/gpu_profile.sh <commit id>'
OUT=${OUT:-runs}; mkdir -p $OUT
export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
cd /tmp
timeout 200 rocprofv3 --kernel-trace --stats --output-format csv -d $R/$OUT/prof -o r1 -- python $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-fp32-leg --no-extra > $R/$OUT/prof_bench.json 2> $R/$OUT/prof.err
timeout 200 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $R/$OUT/pmc_fetch -o f -- python $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-fp32-leg --no-extra > $R/$OUT/pmc_fetch.json 2> $R/$OUT/pmc_fetch.err
timeout 200 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $R/$OUT/pmc_write -o w -- python $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-fp32-leg --no-extra > $R/$OUT/pmc_write.json 2> $R/$OUT/pmc_write.err
cd $R
ls $OUT/pmc_fetch $OUT/pmc_write
python tools/pmc_summary.py $(ls $OUT/pmc_fetch/*counter_collection.csv | head -1) $OUT/pmc_fetch_summary.csv
python tools/pmc_summary.py $(ls $OUT/pmc_write/*counter_collection.csv | head -1) $OUT/pmc_write_summary.csv
python tools/traffic_json.py $OUT/pmc_fetch_summary.csv $OUT/pmc_write_summary.csv $OUT/traffic.json "${1:-unknown}" "$(hostname)" "rocprofv3 --pmc FETCH_SIZE|WRITE_SIZE -- python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-fp32-leg --no-extra"
rm -f $OUT/pmc_fetch/*counter_collection.csv $OUT/pmc_write/*counter_collection.csv $OUT/prof/*kernel_trace.csv
echo "=== stats"; head -25 $OUT/prof/r1_kernel_stats.csv
cat $OUT/prof_bench.json
