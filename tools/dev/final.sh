ulimit -c 0; OUT=${1:?usage: tools/dev/final.sh OUTPUT_DIR}; mkdir -p "$OUT"
timeout -k 10 900 python -m pytest tests -m gpu -x -q > "$OUT/r3_tf.txt" 2>&1; echo "pytest rc=$?" >> "$OUT/r3_tf.txt"; tail -3 "$OUT/r3_tf.txt"
timeout -k 10 300 python __graft_entry__.py --smoke 2>&1 | tail -1
timeout -k 10 600 python bench.py --full > "$OUT/r3_bench4.json" 2> "$OUT/r3_bench4.err"; echo "bench rc=$?"
