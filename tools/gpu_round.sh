#!/bin/bash
# One GPU-box visit.  usage: OUT=<log dir> gpu_round.sh TAG "stage stage ..."   stages: tests smoke bench prof pmc
# Every log lands in $OUT.  Every GPU step runs under its own time limit; the visit ends at the first stage that exits non-zero
# (a fault, an abort or a time limit included) and starts no further GPU process.
R="${GRAFT_REPO_ROOT:-/root/repo}"
cd "$R"
OUT="${OUT:?set OUT to the directory the logs go to}"
mkdir -p "$OUT" && OUT="$(cd "$OUT" && pwd)"       # a relative OUT is under the repository root
TAG=${1:-r1}
STAGES=${2:-"tests smoke bench prof"}
TESTSEL=${3:-tests}
export TMPDIR=/tmp
lscpu | grep -E "Model name|^CPU\(s\)" > $OUT/${TAG}_env.log

stop_on_failure() {   # stage name, exit status, log
  if [ "$2" -ne 0 ]; then
    echo "$1 exited $2: ending the visit here, no further GPU step is started" | tee -a "$3"
    exit "$2"
  fi
}

for S in $STAGES; do
  case $S in
    tests)
      timeout -k 10 900 python -m pytest $TESTSEL -m gpu -q --tb=short -p no:cacheprovider -s > $OUT/${TAG}_tests.log 2>&1
      rc=$?; echo "pytest exit $rc" >> $OUT/${TAG}_tests.log
      tail -4 $OUT/${TAG}_tests.log
      stop_on_failure tests $rc $OUT/${TAG}_tests.log ;;
    smoke)
      timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/${TAG}_smoke.log 2>&1
      rc=$?; echo "smoke exit $rc" >> $OUT/${TAG}_smoke.log
      tail -2 $OUT/${TAG}_smoke.log
      stop_on_failure smoke $rc $OUT/${TAG}_smoke.log ;;
    bench)
      timeout -k 10 600 python bench.py --full --steps 3 --warmup 1 > $OUT/${TAG}_bench.log 2>&1
      rc=$?; echo "bench exit $rc" >> $OUT/${TAG}_bench.log
      tail -3 $OUT/${TAG}_bench.log
      stop_on_failure bench $rc $OUT/${TAG}_bench.log ;;
    prof)
      cd /tmp
      timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_${TAG} -o ${TAG} -- python $R/bench.py --full --steps 1 --warmup 0 --no-cpu-baseline --no-roofline --no-ttfs --no-parity-mode --no-configs --no-slot-pool --no-ids-check > $OUT/${TAG}_rocprof.log 2>&1
      rc=$?; echo "rocprof exit $rc" >> $OUT/${TAG}_rocprof.log
      find /tmp/prof_${TAG} -name "*stats*.csv" -exec cp {} $OUT/ \;
      find /tmp/prof_${TAG} -type f >> $OUT/${TAG}_rocprof.log
      cd "$R"
      stop_on_failure prof $rc $OUT/${TAG}_rocprof.log ;;
    pmc)
      # one pass per counter, with plain blocking polls from the start: the profiler has crashed under the pinned-memory polls
      cd /tmp
      for C in FETCH_SIZE WRITE_SIZE; do
        CTTS_SYNC_POLL=1 timeout -k 10 300 rocprofv3 --kernel-trace --pmc $C --output-format csv -d /tmp/pmc_${TAG}_$C -o ${TAG}_$C -- python $R/bench.py --full --steps 1 --warmup 0 --no-cpu-baseline --no-roofline --no-ttfs --no-parity-mode --no-configs --no-slot-pool --no-ids-check > $OUT/${TAG}_pmc_$C.log 2>&1
        rc=$?; echo "rocprof exit $rc" >> $OUT/${TAG}_pmc_$C.log
        stop_on_failure "pmc $C" $rc $OUT/${TAG}_pmc_$C.log
      done
      python $R/tools/pmc_summary.py /tmp/pmc_${TAG}_FETCH_SIZE /tmp/pmc_${TAG}_WRITE_SIZE $OUT/${TAG}_pmc_traffic.json > $OUT/${TAG}_pmc_summary.txt 2>&1
      cd "$R" ;;
  esac
done
