# GPU round check: every GPU test, smoke, the full bench (run from the repo
# root on the GPU box; logs go to $OUT, default round_out/)
set -o pipefail
OUT=${OUT:-round_out}
mkdir -p "$OUT"
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > "$OUT/pytest_gpu.log" 2>&1 || exit 1
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1 || exit 1
timeout -k 10 600 python bench.py --full > "$OUT/bench.log" 2>&1
