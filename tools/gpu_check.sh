#!/bin/bash
# GPU round trip: parity tests, bench, rocprofv3 kernel stats. Every GPU step has its own limit;
# the chain stops at the first failure.
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
mkdir -p gpurun_out/prof
O="$PWD/${_%/prof}"; R="$PWD"   # the directory made above, absolute; the repository root
timeout -k 10 600 python -m pytest tests -m gpu -q --timeout 300 > gpurun_out/pytest_gpu.log 2>&1 || { tail -40 gpurun_out/pytest_gpu.log; exit 1; }
grep -E "passed|failed" gpurun_out/pytest_gpu.log | tail -1
timeout -k 10 400 python bench.py --full --steps 5 --warmup 2 ${BENCH_ARGS:---no-cpu-baseline} > "$O/bench.json" 2> "$O/bench.err" || { tail -20 "$O/bench.err"; exit 1; }
cat gpurun_out/bench.json
if [ -n "$PROFILE" ]; then
  cd /tmp && export TMPDIR=/tmp
  timeout -k 10 400 rocprofv3 --kernel-trace --stats -d "$O/prof" -o run --output-format csv -- python3 "$R/bench.py" --full --steps 3 --warmup 1 --no-cpu-baseline > "$O/prof_bench.json" 2> "$O/prof_bench.err" || exit 1
fi
