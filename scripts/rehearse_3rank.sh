# one-GPU rehearsal of the driver's command at the reference's own world size (3 ranks, sw/run.sh: mpirun -n 3), with
# its gates and extras (--full). Logs go to $OUT_DIR (default bench_logs/r6o).
set -e
OUT=${OUT_DIR:-bench_logs/r6o}
mkdir -p "$OUT"
timeout -k 10 600 python3 bench.py --gpus 3 --steps 10 --warmup 3 --full > "$OUT"/g3.log 2>&1
grep -o '"ms_per_step": [0-9.]*' "$OUT"/g3.log | head -1; grep -o '"gates_failed": [^]]*]' "$OUT"/g3.log | head -1
