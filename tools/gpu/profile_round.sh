# Full GPU round: parity suite, smoke, the full bench (whole-batch parity + CPU
# baseline), kernel-trace stats of a plain bench, and one rocprofv3 --pmc pass
# per counter (separate runs).  Run from the repo root on the GPU box; logs go
# to $OUT, default round_out/.
set -o pipefail
OUT=${OUT:-round_out}
mkdir -p "$OUT"
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > "$OUT/pytest_gpu.log" 2>&1 || exit 1
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1 || exit 1
timeout -k 10 600 python bench.py --full > "$OUT/bench.log" 2>&1 || exit 1
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT/prof" -o run --output-format csv -- python bench.py > "$OUT/bench_prof.log" 2>&1 || exit 1
for c in FETCH_SIZE WRITE_SIZE TCC_EA0_RDREQ_sum; do
  timeout -s KILL 300 rocprofv3 --pmc $c -d "$OUT/pmc_$c" -o run --output-format csv -- python bench.py --steps 5 > "$OUT/pmc_$c.log" 2>&1 || exit 1
done
