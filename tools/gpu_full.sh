#!/bin/bash
# The whole -m gpu suite, smoke(), then the bench with every side record (--full, PMC child included).
cd "$(dirname "$0")/.."
OUT=${OUT:-results}
mkdir -p "$OUT"
timeout -k 10 1500 python -m pytest tests/ -q -m gpu -p no:cacheprovider > "$OUT/full_tests.log" 2>&1
rc=$?
echo "pytest rc=$rc"; grep -E "passed|failed|FAILED|Error" "$OUT/full_tests.log" | tail -20
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then tail -40 "$OUT/full_tests.log"; exit $rc; fi
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1
echo "smoke rc=$?"; tail -5 "$OUT/smoke.log"
timeout -k 10 900 python bench.py --full > "$OUT/bench_full.json" 2> "$OUT/bench_full.err"
echo "bench rc=$?"; tail -c 6000 "$OUT/bench_full.json"; tail -5 "$OUT/bench_full.err"
