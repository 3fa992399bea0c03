# Round-6 late check of the current tree on one box: GPU suite, smoke, the driver's N=1 command with everything it
# measures (--full), and a kernel trace of the flagship and the MB 1792 step (per-kernel breakdown with
# tools/step_breakdown.py). Logs go to $OUT_DIR (default bench_logs/r6g).
set -e
OUT=${OUT_DIR:-bench_logs/r6g}
mkdir -p "$OUT"
export TMPDIR=/tmp
timeout -k 10 600 python3 -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > "$OUT"/suite.log 2>&1
timeout -k 10 200 python3 -c "import __graft_entry__ as g; g.smoke()" > "$OUT"/smoke.log 2>&1
timeout -k 10 400 python3 bench.py --steps 20 --warmup 5 --full > "$OUT"/bench_driver.log 2>&1
timeout -k 10 200 rocprofv3 --kernel-trace --stats -d "$OUT"/prof8192 -o run --output-format csv -- python3 bench.py --steps 20 --warmup 5 > "$OUT"/prof8192.log 2>&1
timeout -k 10 200 rocprofv3 --kernel-trace --stats -d "$OUT"/prof1792 -o run --output-format csv -- python3 bench.py --mb-per-gpu 1792 --steps 20 --warmup 5 > "$OUT"/prof1792.log 2>&1
tail -n 2 "$OUT"/suite.log; tail -n 1 "$OUT"/smoke.log
grep -o '"ms_per_step": [0-9.]*' "$OUT"/bench_driver.log | head -1
