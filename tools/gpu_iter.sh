#!/bin/bash
# quick GPU iteration: parity tests + short bench (+ optional kernel trace of the --full bench); a failing step ends the script
# usage: tools/gpu_iter.sh <output dir>      BENCH_ARGS: more bench.py arguments; PROFILE=1: the kernel trace
[ -n "$1" ] || { echo "usage: tools/gpu_iter.sh <output dir>" >&2; exit 2; }
R=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$1" && O=$(cd "$1" && pwd) || exit 1
cd "$R"
export TMPDIR=/tmp
timeout -k 10 900 python -m pytest tests -m gpu -x -q > $O/pytest_gpu.log 2>&1; rc=$?; echo "pytest rc=$rc"
tail -15 $O/pytest_gpu.log
[ $rc -eq 0 ] || exit $rc
timeout -k 10 600 python bench.py --steps 100 --warmup 10 ${BENCH_ARGS} > $O/bench.log 2> $O/bench.err; rc=$?; echo "bench rc=$rc"
cat $O/bench.log; tail -5 $O/bench.err
[ $rc -eq 0 ] || exit $rc
if [ -n "$PROFILE" ]; then
  cd /tmp && timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $O/prof_bench --output-format csv -- python3 $R/bench.py --steps 100 --warmup 10 --full --no-cpu-baseline > $O/prof_bench.log 2>&1; rc=$?; echo "rocprof rc=$rc"
  exit $rc
fi
