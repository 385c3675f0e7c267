#!/bin/bash
# GPU box: TP tests + a 2-rank shared-GPU rehearsal of bench.py with the one-shot collective
OUT=${OUT:-results}
mkdir -p "$OUT"
python -c "import __graft_entry__ as g; g.build()" > "$OUT/build.log" 2>&1
timeout -k 10 600 python -m pytest tests/test_gpu_tp_processes.py tests/test_gpu_tp.py -x -q -m gpu > "$OUT/tp_tests.log" 2>&1 || { tail -30 "$OUT/tp_tests.log"; exit 1; }
tail -2 "$OUT/tp_tests.log"
timeout -k 10 600 python bench.py --full --gpus 2 --model 7b --steps 16 --warmup 4 --no-extras > "$OUT/bench_tp2_oneshot.json.log" 2> "$OUT/bench_tp2_oneshot.err" || { tail -20 "$OUT/bench_tp2_oneshot.err"; exit 1; }
tail -c 3000 "$OUT/bench_tp2_oneshot.json.log"
timeout -k 10 600 python bench.py --full --gpus 2 --model 7b --steps 16 --warmup 4 --no-extras --collective rccl > "$OUT/bench_tp2_gloo.json.log" 2> "$OUT/bench_tp2_gloo.err" || { tail -20 "$OUT/bench_tp2_gloo.err"; exit 1; }
tail -c 1500 "$OUT/bench_tp2_gloo.json.log"
