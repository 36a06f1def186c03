#!/usr/bin/env python3
"""A/B of get_rows with u32 and with u16 labels (mbrwt_get_rows_device_async
against mbrwt_get_rows16_device_async) on the synthetic contexts of bench.py:

    python tools/bench_rows16.py                    # C4: 3.7 G x 2,652, 8 M rows a step
    python tools/bench_rows16.py --workload c3      # C3: 1 G x 3,173, 10 M rows a step
    python tools/bench_rows16.py --host             # + mbrwt_get_rows against mbrwt_get_rows16, pinned buffers

Both widths run in one process on the same context, the same batches and the
same streams, in alternating legs (u32, u16, u32, u16, ...) of --steps
asynchronous steps each, after a warm-up of both; a leg is timed by device
events.  One query stream, then two (batch i on context i mod 2, as bench.py).
After the timed loops every batch's whole u16 CSR is compared with its u32 CSR
element by element (bench.py --full pins the u32 batch to the oracle).  The
last output line is one JSON object with every figure.  Needs a GPU: without
one the tool exits with an error (there is no CPU timing).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# bench.py's WORKLOADS (BASELINE.json C4 and C3)
WORKLOADS = {
    "c4": dict(rows=3_700_000_000, cols=2652, density=0.003, batch=8_000_000),
    "c3": dict(rows=1_000_000_000, cols=3173, density=0.038, batch=10_000_000),
}


def parse():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="c4")
    ap.add_argument("--rows", type=int, default=None)
    ap.add_argument("--cols", type=int, default=None)
    ap.add_argument("--density", type=float, default=None)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--arity", type=int, default=8)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--batches", type=int, default=4, help="distinct batches of random rows (step i: batch i mod K)")
    ap.add_argument("--steps", type=int, default=20, help="steps per leg (at least 20)")
    ap.add_argument("--legs", type=int, default=5, help="legs per width (alternating u32, u16)")
    ap.add_argument("--warmup", type=int, default=5, help="warm-up steps per width")
    ap.add_argument("--streams", default="1,2", help="query streams to measure, e.g. 1,2")
    ap.add_argument("--host", action="store_true", help="also time the host-buffer calls on pinned buffers")
    ap.add_argument("--host-reps", type=int, default=3)
    a = ap.parse_args()
    for k, v in WORKLOADS[a.workload].items():
        if getattr(a, k) is None:
            setattr(a, k, v)
    if a.steps < 20:
        ap.error("--steps: at least 20 steps per leg")
    if a.legs < 2:
        ap.error("--legs: at least 2 legs per width")
    a.streams = sorted({int(x) for x in a.streams.split(",")})
    if not a.streams or min(a.streams) < 1 or max(a.streams) > 4:
        ap.error("--streams: 1 .. 4 query streams")
    return a


def log(msg):
    print(msg, flush=True)


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "legs": xs}


def main():
    a = parse()
    try:
        import torch
        gpu = torch.cuda.is_available()
    except Exception:  # noqa: BLE001
        gpu = False
    if not gpu:
        sys.exit("bench_rows16: needs a GPU (no CPU timing is printed)")
    from genome_graph_annotation_amd import BRWTDevice, _lib as L

    dev_t = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    t0 = time.time()
    mat = BRWTDevice.synthetic(a.rows, a.cols, a.density, a.arity, a.seed, device=0, layout="rows")
    log(f"{a.workload}: {a.rows} x {a.cols}, density {a.density}: built in {time.time() - t0:.1f} s, "
        f"{mat.device_bytes() / 1e9:.1f} GB, kernel {mat.traverse_kernel()}, {mat.rows_stats()}")
    K, n = max(1, a.batches), a.batch
    batches_np = [np.random.default_rng(a.seed + k).integers(0, a.rows, n, dtype=np.uint64) for k in range(K)]
    rows_ts = [torch.from_numpy(b.view(np.int64)).to(dev_t) for b in batches_np]
    main_s = torch.cuda.current_stream(dev_t)
    # the label buffers, sized once by the capacity protocol
    off0 = torch.empty(n + 1, dtype=torch.int64, device=dev_t)
    needs = []
    for rt in rows_ts:
        try:
            needs.append(mat.get_rows16_device(rt, off0, None, main_s.cuda_stream))
        except L.MBRWTError as e:
            if e.status != L.MBRWT_ERR_CAPACITY:
                raise
            needs.append(e.needed)
    cap = int(max(needs) * 1.02) + 1024
    log(f"batch {n} rows, {K} batches, labels per batch {needs}")

    Qmax = max(a.streams)
    qmats, qstreams = [mat], [torch.cuda.Stream(dev_t)]
    for _ in range(Qmax - 1):
        qmats.append(mat.clone())
        qstreams.append(torch.cuda.Stream(dev_t))
    offs = [off0] + [torch.empty_like(off0) for _ in range(Qmax - 1)]
    cols = {4: [torch.empty(cap, dtype=torch.int32, device=dev_t) for _ in range(Qmax)],
            2: [torch.empty(cap, dtype=torch.int16, device=dev_t) for _ in range(Qmax)]}
    status = {w: [torch.zeros(3, dtype=torch.int64, device=dev_t) for _ in range(Qmax)] for w in (4, 2)}

    def step(i, Q, width):
        q = i % Q
        call = qmats[q].get_rows_device_async if width == 4 else qmats[q].get_rows16_device_async
        call(rows_ts[i % K], offs[q], cols[width][q], status[width][q], qstreams[q].cuda_stream)

    def leg(Q, width, steps):
        """ms per step of `steps` asynchronous steps on Q streams, between device events."""
        torch.cuda.synchronize()
        start = torch.cuda.Event(enable_timing=True)
        ends = [torch.cuda.Event(enable_timing=True) for _ in range(Q)]
        start.record(qstreams[0])
        for q in range(1, Q):
            qstreams[q].wait_event(start)
        for i in range(steps):
            step(i, Q, width)
        for q in range(Q):
            ends[q].record(qstreams[q])
        torch.cuda.synchronize()
        return max(start.elapsed_time(e) for e in ends) / steps

    def check_status():
        for w in (4, 2):
            for st in status[w]:
                need_l, st_l, sticky = st.cpu().tolist()
                if sticky not in (0, 1 << L.MBRWT_OK):
                    raise RuntimeError(f"asynchronous get_rows (width {w}) reported status bits {sticky:#x} "
                                       f"(last status {st_l}, labels {need_l})")

    result = {"workload": a.workload, "rows": a.rows, "cols": a.cols, "density": a.density, "batch": n,
              "labels_per_batch": needs, "steps_per_leg": a.steps, "legs": a.legs,
              "kernel": mat.traverse_kernel(), "streams": {}}
    for Q in a.streams:
        for w in (4, 2):
            leg(Q, w, a.warmup)
        t = {4: [], 2: []}
        for _ in range(a.legs):   # A B A B ...
            t[4].append(leg(Q, 4, a.steps))
            t[2].append(leg(Q, 2, a.steps))
        check_status()
        r = {}
        for w, name in ((4, "u32"), (2, "u16")):
            r[name] = dict(spread(t[w]), rows_per_s=n / (statistics.median(t[w]) * 1e-3))
            log(f"streams {Q} {name}: {r[name]['median']:.4f} ms/step (legs {min(t[w]):.4f} .. {max(t[w]):.4f}), "
                f"{r[name]['rows_per_s'] / 1e9:.3f} G rows/s")
        r["u16_over_u32"] = r["u16"]["median"] / r["u32"]["median"]
        result["streams"][str(Q)] = r

    # the whole batches, element by element
    equal = True
    s0 = qstreams[0]
    for k in range(K):
        o32, o16 = offs[0], torch.empty_like(offs[0])
        for w in (4, 2):
            status[w][0].zero_()
        qmats[0].get_rows_device_async(rows_ts[k], o32, cols[4][0], status[4][0], s0.cuda_stream)
        qmats[0].get_rows16_device_async(rows_ts[k], o16, cols[2][0], status[2][0], s0.cuda_stream)
        torch.cuda.synchronize()
        s32, s16 = status[4][0].cpu().tolist(), status[2][0].cpu().tolist()
        if s32 != [needs[k], L.MBRWT_OK, 1] or s16 != s32:
            raise RuntimeError(f"batch {k}: status blocks {s32} (u32), {s16} (u16), labels {needs[k]}")
        same = torch.equal(o32, o16)
        piece = 1 << 28   # (compared in pieces: no second copy of a 1.2 G-label batch)
        for b in range(0, needs[k], piece):
            e = min(needs[k], b + piece)
            same &= bool(torch.equal(cols[2][0][b:e].to(torch.int32) & 0xFFFF, cols[4][0][b:e]))
        log(f"batch {k}: {needs[k]} labels, u16 == u32: {same}")
        equal &= same
    result["whole_batches_equal"] = equal

    if a.host:
        result["host"] = host_leg(a, mat, batches_np[0], needs[0], dev_t, torch, L)
    print(json.dumps(result), flush=True)
    if not equal:
        sys.exit("bench_rows16: the u16 CSR differs from the u32 CSR")


def pcie_rates(torch, dev_t, mib=256):
    """Pinned H2D / D2H GB/s (copies of `mib` MiB, best of 3), as bench.py measures its PCIe bound."""
    nb = mib << 20
    d = torch.empty(nb, dtype=torch.uint8, device=dev_t)
    h = torch.empty(nb, dtype=torch.uint8).pin_memory()
    out = {}
    for name, fn in (("h2d", lambda: d.copy_(h, non_blocking=True)), ("d2h", lambda: h.copy_(d, non_blocking=True))):
        fn()
        torch.cuda.synchronize()
        best = 0.0
        for _ in range(3):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            best = max(best, nb / (time.perf_counter() - t0) / 1e9)
        out[name + "_GBs"] = best
    return out


def host_leg(a, mat, rows_np, n_labels, dev_t, torch, L):
    """mbrwt_get_rows against mbrwt_get_rows16 on page-locked caller buffers, alternating; best of --host-reps."""
    lib = L.lib()
    n = len(rows_np)
    rates = pcie_rates(torch, dev_t)
    r = torch.from_numpy(rows_np.view(np.int64)).pin_memory()
    o = {w: torch.empty(n + 1, dtype=torch.int64).pin_memory() for w in (4, 2)}
    c = {4: torch.empty(max(1, n_labels), dtype=torch.int32).pin_memory(),
         2: torch.empty(max(1, n_labels), dtype=torch.int16).pin_memory()}
    fn = {4: (lib.mbrwt_get_rows, C.c_uint32), 2: (lib.mbrwt_get_rows16, C.c_uint16)}
    times = {4: [], 2: []}
    for i in range(a.host_reps + 1):
        for w in (4, 2):
            f, ct = fn[w]
            need = C.c_uint64(0)
            t0 = time.perf_counter()
            st = f(mat._h, C.cast(C.c_void_p(r.data_ptr()), C.POINTER(C.c_uint64)), n,
                   C.cast(C.c_void_p(o[w].data_ptr()), C.POINTER(C.c_uint64)),
                   C.cast(C.c_void_p(c[w].data_ptr()), C.POINTER(ct)), n_labels, C.byref(need))
            dt = time.perf_counter() - t0
            if st != L.MBRWT_OK or need.value != n_labels:
                raise RuntimeError(f"host call (width {w}): status {st}, labels {need.value}")
            if i:
                times[w].append(dt)
    same = bool(torch.equal(o[4], o[2])) and bool(torch.equal(c[2][:n_labels].to(torch.int32) & 0xFFFF,
                                                                c[4][:n_labels]))
    out = {"rows": n, "labels": n_labels, "pcie": rates, "equal": same}
    for w, name in ((4, "u32"), (2, "u16")):
        bytes_in, bytes_out = 8 * n, 8 * (n + 1) + w * n_labels
        bound = max(bytes_in / (rates["h2d_GBs"] * 1e9), bytes_out / (rates["d2h_GBs"] * 1e9))
        best = min(times[w])
        out[name] = {"ms": best * 1e3, "rows_per_s": n / best, "ms_all": [t * 1e3 for t in times[w]],
                     "bytes_per_row": (bytes_in + bytes_out) / n, "pcie_bound_ms": bound * 1e3,
                     "pcie_bound_rows_per_s": n / bound, "vs_pcie_bound": best / bound}
        log(f"host pinned {name}: {best * 1e3:.1f} ms, {n / best / 1e6:.1f} M rows/s, "
            f"{out[name]['bytes_per_row']:.1f} B/row over PCIe, {best / bound:.2f} x its PCIe bound "
            f"({n / bound / 1e6:.1f} M rows/s)")
    if not same:
        raise RuntimeError("host call: the u16 CSR differs from the u32 CSR")
    return out


if __name__ == "__main__":
    main()
