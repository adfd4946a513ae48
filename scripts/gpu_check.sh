#!/bin/bash
# GPU round trip: parity tests, bench line, kernel stats.  bash scripts/gpu_check.sh [bench args...]
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=${MPC_OUT:-$R/bench_out}
mkdir -p $OUT
cd $R
timeout -k 10 600 python -m pytest tests -m gpu -x -q > $OUT/t.log 2>&1
rc=$?
tail -3 $OUT/t.log
[ $rc -eq 0 ] || { grep -E "^E |Error" $OUT/t.log | head -20; exit $rc; }
timeout -k 10 300 python bench.py --full --steps 20 --warmup 5 "$@" > $OUT/b.log 2>&1 || { tail -20 $OUT/b.log; exit 1; }
grep metric $OUT/b.log
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof -o run --output-format csv -- python3 $R/bench.py --full --steps 20 --warmup 5 --no-cpu-baseline > $OUT/p.log 2>&1 || { tail -20 $OUT/p.log; exit 1; }
python3 $R/scripts/kstats.py $OUT/prof 14
