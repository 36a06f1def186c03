"""mbrwt_get_columns_device against a loop of mbrwt_get_column_device (the
only way to the same result without it), in one process on the C2 structure
(1 M rows x 2,652 columns, density 0.3 %, arity 8, library defaults).

Per n_columns in {1, 8, 64, 2652}, over the whole matrix: every result is
first checked against the loop's, then both are timed with HIP events around
the calls -- the median of --reps after one warm-up.  The sizing call (rows =
NULL: the count sweep and the offsets alone) is timed too; the filling call
less the sizing call is the emit sweep with its scan, sort and scatter.  For
2,652 columns the loop is timed on a 64-column sample and scaled (stated in
the output).  Prints one JSON line per n_columns; --out appends them to a log.

    python tools/bench_get_columns.py --out profiles/get_columns/c2.log
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--columns", type=int, default=2652)
    ap.add_argument("--density", type=float, default=0.003)
    ap.add_argument("--arity", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=64, help="columns of the loop's sample at n_columns > sample")
    ap.add_argument("--n-columns", default=None, help="comma-separated n_columns instead of 1,8,64,all")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from genome_graph_annotation_amd import BRWTDevice, MBRWTError

    dev = BRWTDevice.synthetic(a.rows, a.columns, a.density, arity=a.arity, seed=42)
    n, m = dev.num_rows(), dev.num_columns()
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    rng = np.random.default_rng(1)
    lines = [json.dumps({"structure": {"rows": n, "columns": m, "density": a.density, "arity": a.arity,
                                       "layout": dev.layout(), "relations": dev.num_relations(),
                                       "device_bytes": dev.device_bytes()},
                         "device": torch.cuda.get_device_name(0), "reps": a.reps})]
    print(lines[0], flush=True)

    def timed(fn):
        fn()  # warm-up (workspaces grown)
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms)

    col_buf = torch.empty(n, dtype=torch.int64, device="cuda")
    for k in ([int(v) for v in a.n_columns.split(',')] if a.n_columns else (1, 8, 64, m)):
        columns = None if k == m else np.sort(rng.choice(m, k, replace=False)).astype(np.uint64)
        ids = np.arange(m, dtype=np.uint64) if columns is None else columns
        off_t = torch.zeros(k + 1, dtype=torch.int64, device="cuda")
        try:
            total = dev.get_columns_device(columns, 0, n, off_t, None, s)
        except MBRWTError as e:
            total = e.needed
        rows_t = torch.empty(max(1, total), dtype=torch.int64, device="cuda")
        assert dev.get_columns_device(columns, 0, n, off_t, rows_t, s) == total
        torch.cuda.synchronize()
        off = off_t.cpu().numpy().view(np.uint64)
        rows = rows_t.cpu().numpy().view(np.uint64)
        # the check: every slot == the loop's column
        for j, c in enumerate(ids):
            got = dev.get_column_device(int(c), col_buf, s)
            torch.cuda.synchronize()
            assert np.array_equal(col_buf[:got].cpu().numpy().view(np.uint64), rows[int(off[j]):int(off[j + 1])]), c
        # (the loop is timed on a sample of the columns where there are many)
        sample = ids if k <= a.sample else np.sort(rng.choice(ids, a.sample, replace=False))

        def batched():
            dev.get_columns_device(columns, 0, n, off_t, rows_t, s)

        def sizing():
            try:
                dev.get_columns_device(columns, 0, n, off_t, None, s)
            except MBRWTError:
                pass

        def loop():
            for c in sample:
                dev.get_column_device(int(c), col_buf, s)

        t_b, t_s, t_l = timed(batched), timed(sizing), timed(loop)
        scale = k / len(sample)
        line = json.dumps({"n_columns": k, "result_rows": int(total), "get_columns_ms": round(t_b, 3),
                           "sizing_call_ms": round(t_s, 3), "emit_ms": round(t_b - t_s, 3),
                           "loop_ms": round(t_l * scale, 3), "loop_columns_timed": len(sample),
                           "loop_scaled": scale != 1, "speedup": round(t_l * scale / t_b, 2)})
        print(line, flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    dev.close()


if __name__ == "__main__":
    main()
