"""The measurement panda_lookup_multiplicities / panda_poly_running_sum stand on.  There is no earlier way to do either step on the
device, so the yardstick is the stream floor on the same device in the same run: a device-to-device panda_memcpy that moves as many
bytes as the call reads and writes (a copy of B bytes reads B and writes B, so B = (bytes read + bytes written) / 2: for the lookup the
table, the columns and the multiplicities; for the running sum one vector, half of one for the totals alone).
  lookup    arm M: the copy;  arm L: panda_lookup_multiplicities;  arm m: the copy again (the A/A of the baseline)
            distributions of the column values: "uniform" over the table, "constant" (every value one table row: what padding rows
            look like, the case the probe's per-wave combining is for), "misses" (uniform, 10 % of the values absent from the table)
  sum       arm M: the copy;  arm S: panda_poly_running_sum out of place;  arm s: in place;  arm T: totals only (copy of half);  arm m
Before anything is timed the outputs are compared: `missing` with the planted count and the rows with a non-zero multiplicity with the
rows the host drew (numpy bincount); the running sum through the CPU oracle by out_(i+1) = out_i + in_i (up to --verify-max elements).
Every shape is warmed up, wall clock around calls that end in a synchronise, the arms alternated --alternations times, each arm timed
over enough calls to last --min-seconds.  Medians, milliseconds per call.  One JSON line per configuration, then a table with the
ratios to the copy, and the two ratios of record: constant against uniform at the largest table, running sum against copy there.

usage: lookup_bench.py [--tables 65536,1048576,16777216] [--columns 1,4] [--sums 65536,1048576,16777216,1048579] [--alternations N]
                       [--min-seconds S] [--out FILE] [--verify-max ELEMS]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from panda_amd import gpu_ffi as ffi  # noqa: E402

FIELD = 0  # BN254 Fr
DISTRIBUTIONS = ("uniform", "constant", "misses")


def device_name():
    try:
        import torch
        p = torch.cuda.get_device_properties(0)
        return f"{p.name} ({getattr(p, 'gcnArchName', '?').split(':')[0]}, {p.multi_processor_count} CUs)"
    except Exception as e:  # noqa: BLE001
        return f"unknown ({type(e).__name__})"


def measure(run, arms, alternations, min_seconds):
    reps = {}
    for arm in arms:  # warm-up of every shape
        run[arm]()
        t0 = time.perf_counter()
        run[arm]()
        reps[arm] = max(1, int(min_seconds / max(time.perf_counter() - t0, 1e-6)) + 1)
    ms = {arm: [] for arm in arms}
    for _ in range(alternations):
        for arm in arms:
            t0 = time.perf_counter()
            for _ in range(reps[arm]):
                run[arm]()
            ms[arm].append((time.perf_counter() - t0) / reps[arm] * 1e3)
    return ms, {arm: statistics.median(ms[arm]) for arm in arms}, reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", default="65536,1048576,16777216")
    ap.add_argument("--columns", default="1,4")
    ap.add_argument("--sums", default="65536,1048576,16777216,1048579")
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--min-seconds", type=float, default=0.1)
    ap.add_argument("--out")
    ap.add_argument("--verify-max", type=int, default=1 << 24)
    a = ap.parse_args()
    import numpy as np
    import oracle as po
    from gpu_util import NULL_STREAM, DeviceBuffer
    from panda_amd import gpu_manager as pgm
    lib = ffi.load()
    gm = pgm.PandaGpuManager(0)
    stream = gm.exec_stream.raw
    out = open(a.out, "a") if a.out else None
    name = device_name()
    recs, lines = [], []

    def emit(rec):
        recs.append(rec)
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def copy_arm(dst, src, nbytes):
        def run():  # a device-to-device copy returns before it has run: the call ends in a synchronise, like the library's
            ffi.check(lib.panda_memcpy(dst.ptr, src.ptr, nbytes), "copy")
            ffi.check(lib.panda_stream_sync(NULL_STREAM), "sync")
        return run

    try:
        tables = [int(x) for x in a.tables.split(",") if x]
        column_counts = [int(x) for x in a.columns.split(",") if x]
        for n_table in tables:
            n, max_cols = n_table, max(column_counts)
            rng = np.random.default_rng(n_table)
            d_table, d_mult = DeviceBuffer(n_table * 32), DeviceBuffer(n_table * 32)
            d_cols = DeviceBuffer(max_cols * n * 32)
            copy_bytes_max = (2 * n_table + max_cols * n) * 16
            d_src, d_dst = DeviceBuffer(copy_bytes_max), DeviceBuffer(copy_bytes_max)
            try:
                ffi.check(lib.panda_gen_scalars(FIELD, 0x7AB + n_table, 0, n_table + 4096, d_src.ptr, NULL_STREAM), "gen")  # the table and 4096 absent values
                ffi.check(lib.panda_stream_sync(NULL_STREAM), "sync")
                ffi.check(lib.panda_memcpy(d_table.ptr, d_src.ptr, n_table * 32), "copy")
                pool = d_src.to_host(np.uint32, nbytes=(n_table + 4096) * 32).reshape(-1, 8)
                table, absent = pool[:n_table], pool[n_table:]
                for dist in DISTRIBUTIONS:
                    idx = rng.integers(0, n_table, (max_cols, n)) if dist != "constant" else np.full((max_cols, n), n_table // 3)
                    lost = rng.random((max_cols, n)) < 0.1 if dist == "misses" else np.zeros((max_cols, n), bool)
                    for c in range(max_cols):
                        col = table[idx[c]]
                        col[lost[c]] = absent[rng.integers(0, 4096, int(lost[c].sum()))]
                        ffi.check(lib.panda_memcpy(C.c_void_p(d_cols.ptr.value + c * n * 32), C.c_void_p(col.ctypes.data), n * 32), "upload")
                        del col
                    for n_columns in column_counts:
                        ptrs = (C.c_void_p * n_columns)(*[d_cols.ptr.value + c * n * 32 for c in range(n_columns)])
                        missing, first = C.c_uint64(0), C.c_uint64(0)

                        def run_lookup():
                            ffi.check(lib.panda_lookup_multiplicities(FIELD, d_table.ptr, n_table, ptrs, n_columns, n, d_mult.ptr, C.byref(missing), C.byref(first), stream),
                                      "multiplicities")

                        run_lookup()
                        found = idx[:n_columns][~lost[:n_columns]]
                        hit_rows = np.flatnonzero(np.bincount(found, minlength=n_table))
                        got_rows = np.flatnonzero(d_mult.to_host(np.uint32).reshape(-1, 8).any(axis=1))
                        if missing.value != int(lost[:n_columns].sum()) or not np.array_equal(hit_rows, got_rows):
                            raise SystemExit(f"table {n_table} x {n_columns} columns, {dist}: wrong multiplicities (missing {missing.value})")
                        copy_bytes = (2 * n_table + n_columns * n) * 16
                        run = {"M": copy_arm(d_dst, d_src, copy_bytes), "L": run_lookup, "m": copy_arm(d_dst, d_src, copy_bytes)}
                        ms, med, reps = measure(run, "MLm", a.alternations, a.min_seconds)
                        ls, sb, la = C.c_uint(0), C.c_size_t(0), C.c_uint(0)
                        ffi.check(lib.panda_lookup_plan(n_table, n_columns, n, C.byref(ls), C.byref(sb), C.byref(la)), "plan")
                        emit({"call": "lookup", "n_table": n_table, "n_columns": n_columns, "n": n, "distribution": dist, "device": name, "log_slots": ls.value,
                              "scratch_bytes": sb.value, "launches": la.value, "missing": missing.value, "copy_bytes": copy_bytes, "calls_per_repetition": reps,
                              "per_call_ms": {arm: [round(v, 5) for v in ms[arm]] for arm in ms}, "median_ms": {arm: round(med[arm], 5) for arm in med},
                              "baseline_spread_ms": round(max(max(ms["M"]) - min(ms["M"]), max(ms["m"]) - min(ms["m"]), abs(med["M"] - med["m"])), 5),
                              "ratio_to_copy": round(med["L"] / med["M"], 3), "copy_gb_per_s": round(2 * copy_bytes / med["M"] / 1e6, 1),
                              "values_g_per_s": round(n_columns * n / med["L"] / 1e6, 3)})
                    del idx, lost
            finally:
                for b in (d_table, d_mult, d_cols, d_src, d_dst):
                    b.free()
        fid = po.FR_OF[FIELD]
        for n in [int(x) for x in a.sums.split(",") if x]:
            nbytes = n * 32
            d_in, d_out, d_work = (DeviceBuffer(nbytes) for _ in range(3))
            tot = np.zeros((1, 8), np.uint32)
            tp = C.c_void_p(tot.ctypes.data)
            try:
                ffi.check(lib.panda_gen_scalars(FIELD, 0x5CE + n, 0, n, d_in.ptr, NULL_STREAM), "gen")
                ffi.check(lib.panda_stream_sync(NULL_STREAM), "sync")
                ffi.check(lib.panda_memcpy(d_work.ptr, d_in.ptr, nbytes), "copy")

                def run_sum(src, to):
                    ffi.check(lib.panda_poly_running_sum(FIELD, src.ptr, to.ptr if to else None, n, 1, tp, stream), "running_sum")

                verified = n <= a.verify_max
                if verified:
                    run_sum(d_in, d_out)
                    x, z, total = d_in.to_host(np.uint32).reshape(n, 8), d_out.to_host(np.uint32).reshape(n, 8), tot.copy()
                    if z[0].any() or not np.array_equal(po.f_vec(fid, po.OP_ADD, z, x), np.concatenate([z[1:], total])):
                        raise SystemExit(f"running sum {n}: not the running sum")
                    run_sum(d_in, None)
                    if not np.array_equal(tot, total):
                        raise SystemExit(f"running sum {n}: the totals alone differ")
                    del x, z
                # the in-place arm runs on a buffer of its own: after the first call it works on earlier outputs, which cost the same
                run = {"M": copy_arm(d_out, d_in, nbytes), "S": lambda: run_sum(d_in, d_out), "s": lambda: run_sum(d_work, d_work), "H": copy_arm(d_out, d_in, nbytes // 2),
                       "T": lambda: run_sum(d_in, None), "m": copy_arm(d_out, d_in, nbytes)}
                ms, med, reps = measure(run, "MSsHTm", a.alternations, a.min_seconds)
                emit({"call": "running_sum", "n": n, "device": name, "verified": verified, "copy_bytes": nbytes, "calls_per_repetition": reps,
                      "per_call_ms": {arm: [round(v, 5) for v in ms[arm]] for arm in ms}, "median_ms": {arm: round(med[arm], 5) for arm in med},
                      "baseline_spread_ms": round(max(max(ms["M"]) - min(ms["M"]), max(ms["m"]) - min(ms["m"]), abs(med["M"] - med["m"])), 5),
                      "ratio_to_copy": {"S": round(med["S"] / med["M"], 3), "s": round(med["s"] / med["M"], 3), "T": round(med["T"] / med["H"], 3)},
                      "copy_gb_per_s": round(2 * nbytes / med["M"] / 1e6, 1), "elements_g_per_s": round(n / med["S"] / 1e6, 3)})
            finally:
                for b in (d_in, d_out, d_work):
                    b.free()
        lines.append("lookup: table rows   columns x n        distribution | copy MiB   M copy ms    m copy ms   spread | lookup ms   x copy | G values/s")
        for r in (r for r in recs if r["call"] == "lookup"):
            lines.append("        %-12d %2d x %-12d %-12s | %8.1f %11.4f %12.4f %8.4f | %9.4f %8.2f | %10.3f" % (
                r["n_table"], r["n_columns"], r["n"], r["distribution"], r["copy_bytes"] / 2**20, r["median_ms"]["M"], r["median_ms"]["m"], r["baseline_spread_ms"],
                r["median_ms"]["L"], r["ratio_to_copy"], r["values_g_per_s"]))
        lines.append("running sum: n        | M copy ms    m copy ms   spread | scan ms    x copy | in place   x copy | half copy ms  totals ms  x half copy | G elem/s")
        for r in (r for r in recs if r["call"] == "running_sum"):
            med, ratio = r["median_ms"], r["ratio_to_copy"]
            lines.append("        %-14d | %9.4f %12.4f %8.4f | %8.4f %8.2f | %8.4f %8.2f | %12.4f %10.4f %12.2f | %8.3f" % (
                r["n"], med["M"], med["m"], r["baseline_spread_ms"], med["S"], ratio["S"], med["s"], ratio["s"], med["H"], med["T"], ratio["T"], r["elements_g_per_s"]))
        big = max(tables) if tables else None
        for n_columns in column_counts:
            pick = {r["distribution"]: r["median_ms"]["L"] for r in recs if r["call"] == "lookup" and r["n_table"] == big and r["n_columns"] == n_columns}
            if "constant" in pick and "uniform" in pick:
                lines.append("constant / uniform at table %d, %d column(s): %.3f" % (big, n_columns, pick["constant"] / pick["uniform"]))
        sums = [r for r in recs if r["call"] == "running_sum"]
        if sums:
            r = max(sums, key=lambda r: r["n"] if r["n"] & (r["n"] - 1) == 0 else 0)
            lines.append("running sum / copy at %d: %.3f" % (r["n"], r["ratio_to_copy"]["S"]))
        text = "\n".join(lines)
        print(text, flush=True)
        if out:
            out.write(text + "\n")
    finally:
        if out:
            out.close()
        gm.deinit()


if __name__ == "__main__":
    main()
