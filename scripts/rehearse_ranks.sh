# one-GPU rehearsals of the driver's multi-rank command (N ranks time-share one GPU; not scaling data): the late
# round-6 tree end to end through the schedule A/B, gates and extras (--full). Logs go to $OUT_DIR (default
# bench_logs/r6k).
set -e
OUT=${OUT_DIR:-bench_logs/r6k}
mkdir -p "$OUT"
timeout -k 10 500 python3 bench.py --gpus 2 --steps 10 --warmup 3 --full > "$OUT"/g2.log 2>&1
timeout -k 10 600 python3 bench.py --gpus ${N4:-4} --steps 10 --warmup 3 --full > "$OUT"/g4.log 2>&1
for f in "$OUT"/g2.log "$OUT"/g4.log; do echo "$f $(grep -o '"ms_per_step": [0-9.]*' $f | head -1) $(grep -o '"gates_failed": [^]]*]' $f | head -1)"; done
