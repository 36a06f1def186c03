"""bench_build.py -- BRWT construction from columns (BRWTBottomUpBuilder::build,
basic partitioner) on the device
(mbrwt_create_from_columns) next to the oracle's CPU restatement of the
reference builder on the same columns (the reference's own mt19937 column
generator, data_generation.cpp:20-29).  Prints one JSON line.  The device
time is end-to-end from host columns to a queryable image (upload,
compute_or + generate_subindex kernels, index columns back to the host, image
layout and upload by build_from_desc); parity: same image size as the
oracle's tree through mbrwt_create and identical get_rows on a row sample."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--cols", type=int, default=2652)
ap.add_argument("--density", type=float, default=0.003)
ap.add_argument("--arity", type=int, default=8)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--relax", type=int, default=0, help="then BRWTOptimizer::relax with this max arity")
ap.add_argument("--from-rows", action="store_true",
                help="the same matrix through from_rows (CSR rows) and from_columns(layout='rows'), reps alternating")
ap.add_argument("--from-sparse-columns", action="store_true",
                help="as --from-rows, with from_sparse_columns (ascending row ids per column) alternating with the two")
ap.add_argument("--greedy", action="store_true",
                help="binary_grouping_greedy instead of the basic partitioner; with --from-rows the shape comes from "
                     "the rows (shape_from_rows) and its steps are timed one by one as well")
a = ap.parse_args()
PART = "greedy" if a.greedy else "basic"

import oracle as O  # checker + CPU baseline only
from genome_graph_annotation_amd import BRWTDevice

n, m = a.rows, a.cols
W = (n + 63) // 64
words = O.generate_columns(n, m, a.density, seed=42)
cols = words[: m * W].reshape(m, W)



def csr_rows(cols, n):
    """The matrix's rows as a CSR (ascending columns per row), from its column words."""
    off = np.zeros(n + 1, dtype=np.uint64)
    parts = []
    for r0 in range(0, n, 1 << 16):
        r1 = min(n, r0 + (1 << 16))
        bits = np.unpackbits(cols[:, r0 // 64:(r1 + 63) // 64].view(np.uint8), axis=1, bitorder="little")
        rr, cc = np.nonzero(bits[:, : r1 - r0].T)
        off[r0 + 1:r1 + 1] = np.bincount(rr, minlength=r1 - r0)
        parts.append(cc.astype(np.uint32))
    return np.cumsum(off, dtype=np.uint64), np.concatenate(parts)


def sparse_columns(cols, n):
    """The matrix's columns as ascending row ids (u32) with their offsets, from its column words."""
    ids = [np.flatnonzero(np.unpackbits(c.view(np.uint8), bitorder="little")[:n]).astype(np.uint32) for c in cols]
    off = np.zeros(len(ids) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(i) for i in ids])
    return off, np.concatenate(ids) if ids else np.zeros(0, dtype=np.uint32)


class LowWater:
    """The low-water mark of hipMemGetInfo's free bytes while the block runs
    (sampled around it and by a thread during it)."""

    def __enter__(self):
        import threading
        import torch
        self._info = lambda: torch.cuda.mem_get_info()[0]
        self.before = self.low = self._info()
        self._stop = threading.Event()

        def poll():
            while not self._stop.is_set():
                self.low = min(self.low, self._info())
                time.sleep(0.0005)
        self._t = threading.Thread(target=poll, daemon=True)
        self._t.start()
        return self

    def __exit__(self, *exc):
        self._stop.set()
        self._t.join()
        self.low = min(self.low, self._info())


if a.from_rows or a.from_sparse_columns:
    import torch
    torch.cuda.init()
    off, lab = csr_rows(cols, n)
    kw = dict(partitioner=PART, relax_max_arity=a.relax)
    build = {"from_rows": lambda: BRWTDevice.from_rows(off, lab, m, arity=a.arity, **kw),
             "from_columns": lambda: BRWTDevice.from_columns(cols, n, a.arity, layout="rows", **kw)}
    names = ["from_rows", "from_columns"]
    if a.from_sparse_columns:
        coff, cids = sparse_columns(cols, n)
        build["from_sparse_columns"] = lambda: BRWTDevice.from_sparse_columns(coff, cids, n, m, arity=a.arity, **kw)
        names.insert(0, "from_sparse_columns")
        few = min(m, 16)
        BRWTDevice.from_sparse_columns(coff[: few + 1], cids[: int(coff[few])], n, few, arity=a.arity, **kw).close()
    BRWTDevice.from_rows(off[:1025], lab[: int(off[1024])], m, arity=a.arity, **kw).close()  # warm-up
    BRWTDevice.from_columns(cols[: min(m, 16)], n, a.arity, layout="rows", **kw).close()
    res = {name: {"s": [], "used": []} for name in names}
    rows = np.random.default_rng(1).integers(0, n, 200_000).astype(np.uint64)
    for _ in range(a.reps):
        for name in names:
            with LowWater() as lw:
                t0 = time.perf_counter()
                built = build[name]()
                res[name]["s"].append(time.perf_counter() - t0)
            res[name]["used"].append(int(lw.before - lw.low))
            res[name]["image_bytes"] = int(built.device_bytes())
            res[name]["stats"] = built.rows_stats()
            res[name]["shape"] = [built.export()[k].tolist() for k in ("num_children", "first_child", "leaf_column")]
            res[name]["rows"] = built.get_rows(rows)
            built.close()
    want = res["from_columns"]
    same = all(r["image_bytes"] == want["image_bytes"] and r["stats"] == want["stats"] and r["shape"] == want["shape"]
               and all(np.array_equal(x, y) for x, y in zip(r["rows"], want["rows"])) for r in res.values())
    steps = {}
    if a.greedy or a.relax:  # the steps of from_rows' shape, each on its own (their sum: one more full run)
        from genome_graph_annotation_amd.brwt import node_counts_from_rows, relax_shape, shape_from_rows
        steps = {"partition_s": [], "counts_s": [], "relax_s": [], "records_s": []}
        for _ in range(a.reps):
            t0 = time.perf_counter()
            plain = shape_from_rows(off, lab, m, PART, a.arity)
            t1 = time.perf_counter()
            counts = node_counts_from_rows(off, lab, m, shape=plain)
            t2 = time.perf_counter()
            shape = relax_shape(plain, counts, a.relax)
            t3 = time.perf_counter()
            BRWTDevice.from_rows(off, lab, m, shape=shape).close()
            t4 = time.perf_counter()
            for k, v in zip(steps, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                steps[k].append(v)
        steps = {k: {"median_s": float(np.median(v)), "runs_s": v} for k, v in steps.items()}
    sparse_steps = {}
    if a.from_sparse_columns and (a.greedy or a.relax):  # the same steps from the sparse columns
        from genome_graph_annotation_amd.brwt import node_counts_from_sparse_columns, shape_from_sparse_columns
        sparse_steps = {"partition_s": [], "counts_s": [], "relax_s": [], "records_s": []}
        for _ in range(a.reps):
            t0 = time.perf_counter()
            plain = shape_from_sparse_columns(coff, cids, n, m, PART, a.arity)
            t1 = time.perf_counter()
            counts = node_counts_from_sparse_columns(coff, cids, n, m, shape=plain)
            t2 = time.perf_counter()
            shape = relax_shape(plain, counts, a.relax)
            t3 = time.perf_counter()
            BRWTDevice.from_sparse_columns(coff, cids, n, m, shape=shape).close()
            t4 = time.perf_counter()
            for k, v in zip(sparse_steps, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                sparse_steps[k].append(v)
        sparse_steps = {k: {"median_s": float(np.median(v)), "runs_s": v} for k, v in sparse_steps.items()}
    print(json.dumps({
        "metric": "row-record build from host data to a queryable context: "
                  + ("from_sparse_columns (ascending row ids per column), " if a.from_sparse_columns else "")
                  + "from_rows (CSR rows) against "
                  "from_columns(layout='rows') (dense columns), reps alternating in one process",
        "config": {"rows": n, "columns": m, "density": a.density, "arity": a.arity, "relations": int(len(lab)),
                   "partitioner": PART, "relax_max_arity": a.relax, "nodes": len(res["from_rows"]["shape"][0])},
        "from_rows_steps": steps,
        **({"from_sparse_columns_steps": sparse_steps} if a.from_sparse_columns else {}),
        **{name: {"median_s": float(np.median(r["s"])), "runs_s": r["s"], "image_bytes": r["image_bytes"],
                  "device_low_water_used_bytes": int(max(r["used"])), "low_water_runs": r["used"]}
           for name, r in res.items()},
        "parity": ("equal shape, image bytes and rows_stats, identical get_rows on 200,000 rows" if same
                   else "MISMATCH"),
    }))
    sys.exit(0 if same else 1)

BRWTDevice.from_columns(cols[: min(m, 16)], n, a.arity, partitioner=PART).close()  # warm-up (HIP init, kernels)
dev_s = []
for _ in range(a.reps):
    t0 = time.perf_counter()
    built = BRWTDevice.from_columns(cols, n, a.arity, relax_max_arity=a.relax, partitioner=PART)
    dev_s.append(time.perf_counter() - t0)
    if _ + 1 < a.reps:
        built.close()
t0 = time.perf_counter()
t = O.OracleTree(O.lib().oracle_build_from_columns(O._p64(words), n, m, int(a.greedy), a.arity, a.relax))
cpu_s = time.perf_counter() - t0
ref = BRWTDevice.from_tree(t.export())
rows = np.random.default_rng(1).integers(0, n, 200_000).astype(np.uint64)
o1, c1 = built.get_rows(rows)
o2, c2 = t.get_rows(rows)
same = built.device_bytes() == ref.device_bytes() and np.array_equal(o1, o2) and np.array_equal(c1, c2)
print(json.dumps({
    "metric": f"BRWT build from columns (BRWTBottomUpBuilder::build, {PART} partitioner"
              + (", then BRWTOptimizer::relax)" if a.relax else ")"),
    "config": {"rows": n, "columns": m, "density": a.density, "arity": a.arity, "relax_max_arity": a.relax,
               "nodes": int(built.num_nodes()),
               "relations": int(built.num_relations()), "image_bytes": int(built.device_bytes())},
    "device_s": float(np.median(dev_s)), "device_runs_s": dev_s,
    "cpu_baseline": {"value_s": cpu_s, "cores": 1, "kind": "port",
                     "sample": "the oracle's restatement of BRWTBottomUpBuilder::build"
                     + (" + BRWTOptimizer::relax" if a.relax else "") + " on the same columns"},
    "parity": ("identical image size to the oracle's tree through mbrwt_create and identical get_rows on "
               "200,000 rows" if same else "MISMATCH"),
}))
