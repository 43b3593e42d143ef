#!/bin/bash
# one rocprofv3 --pmc pass of the C3 bench with the given counters; prints per-kernel means.  usage: OUT=<log dir> pmc_any.sh TAG COUNTER...
R="${GRAFT_REPO_ROOT:-/root/repo}"; cd /tmp; export TMPDIR=/tmp
T=$1; shift
OUT="${OUT:?set OUT to the directory the logs go to}"; OUT="$(cd "$R" && mkdir -p "$OUT" && cd "$OUT" && pwd)"   # a relative OUT is under the repository root
timeout -k 10 900 rocprofv3 --kernel-trace --pmc "$@" --output-format csv -d /tmp/pmc_$T -o $T -- python $R/bench.py --full --steps 1 --warmup 0 --no-cpu-baseline --no-roofline --no-ttfs > $OUT/${T}_run.log 2>&1
rc=$?; if [ $rc -ne 0 ]; then echo "rocprof exit $rc: see $OUT/${T}_run.log"; exit $rc; fi
python - "$T" <<'P' > $OUT/${T}_counters.txt
import csv, glob, sys, collections
f = glob.glob(f"/tmp/pmc_{sys.argv[1]}/**/*counter_collection.csv", recursive=True)[0]
acc = collections.defaultdict(lambda: collections.defaultdict(float)); cnt = collections.Counter()
for r in csv.DictReader(open(f)):
    k = r["Kernel_Name"][:70]; acc[k][r["Counter_Name"]] += float(r["Counter_Value"]); cnt[(k, r["Counter_Name"])] += 1
for k in sorted(acc, key=lambda k: -sum(acc[k].values()))[:14]:
    print(k.ljust(72), "  ".join(f"{c}={acc[k][c] / cnt[(k, c)]:.0f} (n={cnt[(k, c)]})" for c in sorted(acc[k])))
P
cat $OUT/${T}_counters.txt
