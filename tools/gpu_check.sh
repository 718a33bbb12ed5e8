#!/bin/bash
# One GPU session: smoke -> parity tests -> bench -> rocprofv3 kernel stats. Each GPU step has its own
# time limit; test failures (exit 1) continue, anything else (fault/abort/timeout) stops the script.
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
export TMPDIR=/tmp
run() {  # name, limit, cmd...
  local name=$1 lim=$2; shift 2
  echo "== $name" | tee -a $OUT/summary.log
  timeout -k 10 "$lim" "$@" > "$OUT/$name.log" 2>&1
  local rc=$?
  echo "   rc=$rc" | tee -a $OUT/summary.log
  tail -3 "$OUT/$name.log" | tee -a $OUT/summary.log
  if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then echo "stop: $name rc=$rc" | tee -a $OUT/summary.log; exit $rc; fi
  return 0
}
STEPS=${STEPS:-smoke,tests,bench,prof}
[[ $STEPS == *smoke* ]] && run smoke 300 python -c "import __graft_entry__ as g; g.smoke()"
[[ $STEPS == *tests* ]] && run tests 900 python -m pytest tests -m gpu -q -rf
[[ $STEPS == *bench* ]] && run bench 600 python bench.py --full --steps 50 --warmup 5 --cpu-seconds 10
[[ $STEPS == *prof* ]] && run prof 600 rocprofv3 --kernel-trace --stats -d $OUT/prof -o run --output-format csv -- python bench.py --full --steps 20 --warmup 3 --no-cpu-baseline
exit 0
