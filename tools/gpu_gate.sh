#!/bin/bash
# GPU gate of a round: every -m gpu test (verbose failures), then the default bench line.
# usage (from the container): gpurun --timeout 1500 -- 'bash tools/gpu_gate.sh [pytest args]'
OUT=${OUT:-runs}; mkdir -p $OUT
export TMPDIR=/tmp
( time python -m pytest tests -m gpu -q --timeout 900 -rf --durations=15 "$@" ) > $OUT/tests.log 2>&1
echo "=== tests"; tail -60 $OUT/tests.log
( time python bench.py --full ) > $OUT/bench.json 2> $OUT/bench.err
echo "=== bench"; cat $OUT/bench.json; tail -5 $OUT/bench.err
