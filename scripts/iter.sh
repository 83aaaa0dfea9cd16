#!/bin/bash
# One development round trip: selected GPU tests (pytest -k expr), then bench lines.
# usage: bash scripts/iter.sh <tag> "<pytest -k expr>" "<bench args>;<bench args>;..."
set -o pipefail
TAG=$1; K=$2; BENCHES=$3
cd "${GRAFT_REPO_ROOT:-$(pwd)}"
mkdir -p bench_out
if [ -n "$K" ]; then
  timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread -k "$K" \
      > bench_out/${TAG}_test.log 2>&1 || { echo "tests failed rc=$?"; tail -40 bench_out/${TAG}_test.log; exit 1; }
  tail -2 bench_out/${TAG}_test.log
fi
IFS=';' read -ra BS <<< "$BENCHES"
i=0
for b in "${BS[@]}"; do
  [ -z "$b" ] && continue
  timeout -k 10 400 python -u bench.py --full $b > bench_out/${TAG}_bench$i.log 2>&1 \
      || { echo "bench '$b' failed rc=$?"; tail -20 bench_out/${TAG}_bench$i.log; exit 1; }
  echo "== $b"; tail -1 bench_out/${TAG}_bench$i.log | python -c "import json,sys; d=json.loads(sys.stdin.read()); print({k: d.get(k) for k in ('value','ms_per_step','scan_kernel_ms','tail_kernel_ms','pair_kernel_ms','order_ms','hits','survivors','candidates')}, d['roofline']['kernel'], d.get('cpu_baseline',{}).get('parity_vs_gpu'))"
  i=$((i+1))
done
