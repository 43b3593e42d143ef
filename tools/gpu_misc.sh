#!/bin/bash
# documentation runs: BASELINE configs C1/C2/C5, the f32 parity-mode bench line, the continuous-batching probe.  usage: OUT=<log dir> gpu_misc.sh
# Each GPU step runs under its own time limit; the first one that exits non-zero ends the script.
set -o pipefail
cd "$(dirname "$0")/.."; OUT="${OUT:?set OUT to the directory the logs go to}"; mkdir -p "$OUT"
timeout -k 10 600 python tools/configs_run.py > $OUT/configs_run.log 2>&1 && tail -3 $OUT/configs_run.log | cut -c1-300 &&
timeout -k 10 600 python bench.py --full --dtype f32 --steps 2 --warmup 1 --no-cpu-baseline --no-roofline > $OUT/bench_f32.log 2>/dev/null &&
tail -1 $OUT/bench_f32.log | cut -c1-330 &&
timeout -k 10 600 python tools/serving_probe.py > $OUT/serving_probe.log 2>&1 && tail -4 $OUT/serving_probe.log | cut -c1-250
