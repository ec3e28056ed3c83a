#!/bin/bash
# Quick dev session: GPU tests, C2 bench with its side measurements (--full, no
# CPU leg), phase stamps.  Logs go to $OUT_DIR (default measure_out/quick).
set -e
export TMPDIR=/tmp
O=${OUT_DIR:-measure_out/quick}
mkdir -p $O
timeout -k 10 300 python -u -m pytest tests -m gpu -q --timeout 120 --timeout-method thread ${PYTEST_ARGS:-} > $O/pytest_gpu.log 2>&1 || { tail -60 $O/pytest_gpu.log; exit 1; }
tail -3 $O/pytest_gpu.log
timeout -k 10 300 python bench.py --full --no-cpu > $O/bench.log 2>&1 || { tail -30 $O/bench.log; exit 1; }
tail -1 $O/bench.log
timeout -k 10 300 python tools/stamps.py C2 > $O/stamps.log 2>&1 || { tail -30 $O/stamps.log; exit 1; }
cat $O/stamps.log
