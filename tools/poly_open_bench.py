"""The measurement panda_poly_evaluate / panda_poly_divide_linear stand on.  There is no earlier way to do the step on the device, so the
yardstick is the stream floor: a device-to-device panda_memcpy of the same batch x n x 32 bytes, as
  arm M: panda_memcpy, coefficients -> the quotient buffer (reads and writes every byte once);
  arm 1: panda_poly_evaluate at one point;          arm 2: at two points (two sweeps);
  arm D: panda_poly_divide_linear out of place;     arm I: in place;
  arm m: arm M again (the A/A of the baseline: its run-to-run spread in the same alternation).
One process, the arms share their buffers.  Before anything is timed the outputs are compared: in place against out of place byte for
byte, the remainders against the values, and quotient and remainder against the complete characterisation q_(n-1) = 0,
q_(j-1) - z q_j = c_j, r - z q_0 = c_0 by the CPU oracle's vector ops.  Every shape is warmed up, wall clock around calls that end in the
library's own synchronise, the arms alternated M, 1, 2, D, I, m --alternations times, each arm timed over enough calls to last
--min-seconds.  Milliseconds per call.  One JSON line per configuration, then a table with the ratios to the copy.

usage: poly_open_bench.py [--configs field:n:batch,...] [--alternations N] [--min-seconds S] [--out FILE] [--no-verify]"""
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

DEFAULT_CONFIGS = "0:65536:16,0:1048576:16,0:4194304:4,0:16777216:1,0:1048579:16"
FIELD = ("BN254 Fr", "BLS12-377 Fr", "BLS12-381 Fr")
ARMS = "M12DIm"


def device_name():
    try:
        import torch
        p = torch.cuda.get_device_properties(0)
        return f"{p.name} ({getattr(p, 'gcnArchName', '?').split(':')[0]}, {p.multi_processor_count} CUs)"
    except Exception as e:  # noqa: BLE001
        return f"unknown ({type(e).__name__})"


def table(recs):
    lines = ["field         n x batch              MiB   | M copy (min / med / max ms)   | m med    spread  | eval 1 pt  x copy | eval 2 pt  x copy | divide     x copy | in place   x copy | divide GB/s (96 B/elem)  G elem/s"]
    for r in recs:
        med = r["median_ms"]
        lines.append("%-13s %-9d x %-3d %9.1f | %8.4f /%8.4f /%8.4f | %8.4f %7.4f | %9.4f %7.3f | %9.4f %7.3f | %9.4f %7.3f | %9.4f %7.3f | %10.0f %18.2f" % (
            FIELD[r["field"]], r["n"], r["batch"], r["bytes"] / 2**20, *r["M_min_med_max"], med["m"], r["baseline_spread_ms"],
            med["1"], r["ratio_to_copy"]["1"], med["2"], r["ratio_to_copy"]["2"], med["D"], r["ratio_to_copy"]["D"], med["I"], r["ratio_to_copy"]["I"],
            r["divide_gb_per_s"], r["divide_gelem_per_s"]))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=DEFAULT_CONFIGS)
    ap.add_argument("--alternations", type=int, default=10)
    ap.add_argument("--min-seconds", type=float, default=0.2)
    ap.add_argument("--out")
    ap.add_argument("--no-verify", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import oracle as po
    from gpu_util import NULL_STREAM, DeviceBuffer
    from panda_amd import gpu_manager as pgm
    lib = ffi.load()
    gm = pgm.PandaGpuManager(0)
    out = open(a.out, "a") if a.out else None
    recs = []
    name = device_name()
    try:
        for spec in a.configs.split(","):
            field, n, batch = (int(x) for x in spec.split(":"))
            fid = po.FR_OF[field]
            nbytes = batch * n * 32
            pts = po.gen_scalars(fid, 0x90A + n, 2)
            pp = C.c_void_p(pts.ctypes.data)
            coeffs, quot, work = DeviceBuffer(nbytes), DeviceBuffer(nbytes), DeviceBuffer(nbytes)
            vals, rems = np.zeros((batch, 2, 8), np.uint32), np.zeros((batch, 8), np.uint32)
            vp, rp = C.c_void_p(vals.ctypes.data), C.c_void_p(rems.ctypes.data)
            stream = gm.exec_stream.raw
            try:
                ffi.check(lib.panda_gen_scalars(field, 0x0BE + n, 0, batch * n, coeffs.ptr, NULL_STREAM), "gen")
                ffi.check(lib.panda_stream_sync(NULL_STREAM), "sync")
                ffi.check(lib.panda_memcpy(work.ptr, coeffs.ptr, nbytes), "copy")

                def run_copy():
                    ffi.check(lib.panda_memcpy(quot.ptr, coeffs.ptr, nbytes), "copy")

                def run_eval(k):
                    ffi.check(lib.panda_poly_evaluate(field, coeffs.ptr, n, batch, pp, k, vp, stream), "evaluate")

                def run_divide():
                    ffi.check(lib.panda_poly_divide_linear(field, coeffs.ptr, quot.ptr, n, batch, pp, rp, stream), "divide")

                def run_in_place():  # on a buffer of its own: after the first call it divides a quotient, which costs the same
                    ffi.check(lib.panda_poly_divide_linear(field, work.ptr, work.ptr, n, batch, pp, rp, stream), "divide")

                run = {"M": run_copy, "1": lambda: run_eval(1), "2": lambda: run_eval(2), "D": run_divide, "I": run_in_place, "m": run_copy}
                if not a.no_verify:
                    run_in_place()
                    in_place, rem_in_place = work.to_host(np.uint32).reshape(batch, n, 8), rems.copy()
                    run_divide()
                    q = quot.to_host(np.uint32).reshape(batch, n, 8)
                    if not (np.array_equal(q, in_place) and np.array_equal(rems, rem_in_place)):
                        raise SystemExit(f"field {field} {n} x {batch}: in place differs from out of place")
                    run_eval(2)
                    if not np.array_equal(vals[:, 0], rems):
                        raise SystemExit(f"field {field} {n} x {batch}: the value differs from the remainder")
                    c = coeffs.to_host(np.uint32).reshape(batch, n, 8)
                    for p in range(batch):
                        zq = po.f_vec(fid, po.OP_MUL, q[p], np.broadcast_to(pts[0], (n, 8)))
                        ok = not q[p, n - 1].any()
                        ok = ok and np.array_equal(po.f_vec(fid, po.OP_SUB, np.ascontiguousarray(q[p, :n - 1]), np.ascontiguousarray(zq[1:])), c[p, 1:])
                        ok = ok and np.array_equal(po.f_vec(fid, po.OP_SUB, rems[p:p + 1], np.ascontiguousarray(zq[:1]))[0], c[p, 0])
                        if not ok:
                            raise SystemExit(f"field {field} {n} x {batch}: polynomial {p} is not divided correctly")
                    del c, q, in_place
                reps = {}
                for arm in ARMS:  # warm-up of every shape
                    run[arm]()
                    t0 = time.perf_counter()
                    run[arm]()
                    reps[arm] = max(1, int(a.min_seconds / max(time.perf_counter() - t0, 1e-6)) + 1)
                ms = {arm: [] for arm in ARMS}
                for _ in range(a.alternations):
                    for arm in ARMS:
                        t0 = time.perf_counter()
                        for _ in range(reps[arm]):
                            run[arm]()
                        ms[arm].append((time.perf_counter() - t0) / reps[arm] * 1e3)
                med = {arm: statistics.median(ms[arm]) for arm in ARMS}
                spread = max(max(ms["M"]) - min(ms["M"]), max(ms["m"]) - min(ms["m"]), abs(med["M"] - med["m"]))
                tile, chunk, le, ld = C.c_uint(0), C.c_uint(0), C.c_uint(0), C.c_uint(0)
                ffi.check(lib.panda_poly_plan(n, batch, C.byref(tile), C.byref(chunk), C.byref(le), C.byref(ld)), "plan")
                rec = {"field": field, "n": n, "batch": batch, "bytes": nbytes, "device": name, "tile": tile.value, "carry_chunk": chunk.value,
                       "launches_evaluate": le.value, "launches_divide": ld.value, "calls_per_repetition": reps,
                       "per_call_ms": {arm: [round(v, 5) for v in ms[arm]] for arm in ARMS},
                       "median_ms": {arm: round(med[arm], 5) for arm in ARMS},
                       "M_min_med_max": [round(min(ms["M"]), 5), round(med["M"], 5), round(max(ms["M"]), 5)],
                       "baseline_spread_ms": round(spread, 5),
                       "ratio_to_copy": {arm: round(med[arm] / med["M"], 4) for arm in "12DI"},
                       "copy_gb_per_s": round(2 * nbytes / med["M"] / 1e6, 1),
                       "divide_gb_per_s": round(3 * nbytes / med["D"] / 1e6, 1),  # two reads of the coefficients and one write
                       "divide_gelem_per_s": round(batch * n / med["D"] / 1e6, 3)}
                recs.append(rec)
                line = json.dumps(rec)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
            finally:
                for d in (coeffs, quot, work):
                    d.free()
        text = table(recs)
        print(text, flush=True)
        if out:
            out.write(text + "\n")
    finally:
        if out:
            out.close()
        gm.deinit()


if __name__ == "__main__":
    main()
