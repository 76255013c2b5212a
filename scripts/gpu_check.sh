#!/bin/bash
# One GPU-box visit: parity tests, then (only if pytest ended normally) smoke + a short bench.
# usage: scripts/gpu_check.sh <tag> [bench args]
set -u
tag=${1:-run}; shift || true
OUT=${OUT:-out}          # directory of the run's logs and bench lines
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 900 python -m pytest tests -m gpu -q -x --timeout=600 > $OUT/pytest_$tag.log 2>&1
rc=$?
tail -n 25 $OUT/pytest_$tag.log
echo "pytest rc=$rc"
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
timeout -k 10 300 python __graft_entry__.py smoke > $OUT/smoke_$tag.log 2>&1; src=$?
tail -n 3 $OUT/smoke_$tag.log; echo "smoke rc=$src"
if [ $src -ne 0 ] && [ $src -ne 1 ]; then exit $src; fi
timeout -k 10 600 python bench.py --full "$@" > $OUT/bench_$tag.json 2> $OUT/bench_$tag.err; brc=$?
cat $OUT/bench_$tag.err | tail -n 25; cat $OUT/bench_$tag.json; echo "bench rc=$brc"
exit $rc
