"""The measurement panda_poly_evaluate_lagrange / panda_poly_divide_linear_lagrange stand on.  Per configuration
(field, log_n, batch, order) on the subgroup, evaluations generated on the device:
  arm e1 / e4: panda_poly_evaluate_lagrange at one / four points off the domain;
  arm d:       panda_poly_divide_linear_lagrange out of place at a point off the domain;     arm o: the same at a domain point;
against (a) a device-to-device panda_memcpy of each call's own traffic
  arm ce: half the vectors' bytes (an evaluation reads every byte once: a copy of half of them reads and writes as much);
  arm cd: one and a half times the vectors' bytes (a division reads them twice and writes them once);
and (b) the route through coefficients that the library offered before:
  arm b1 / b4: panda_ntt_execute_batch inverse (bit-reversed input for that order) + panda_poly_evaluate at one / four points;
  arm bd:      the inverse transform + panda_poly_divide_linear in place + the forward transform (bit-reversed output for that order).
Route (b) is timed WITHOUT the copy a caller needs who wants to keep the evaluations (the transform overwrites its source), and its
quotient is then in coefficient form only if the forward transform is left out -- which is what the coefficient-form caller wants; arm bd
includes it because the evaluation-form caller does not.  Before anything is timed the values of e1 and b1 are compared byte for byte, and
the quotient of d with that of bd.  Every arm is warmed up, then timed as single synchronous calls, the arms alternated --rounds times;
the figure is the median, milliseconds per call.  One JSON line per configuration, then a table.

usage: poly_lagrange_bench.py [--configs field:log_n:batch,...] [--rounds N] [--out FILE]"""
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

DEFAULT_CONFIGS = "0:16:16,0:20:4,0:24:1,1:20:4,2:20:4"
FIELD = ("BN254 Fr", "BLS12-377 Fr", "BLS12-381 Fr")
ORDER = ("natural", "bitrev")
ARMS = ("ce", "e1", "e4", "b1", "b4", "cd", "d", "o", "bd")


def device_name():
    try:
        import torch
        p = torch.cuda.get_device_properties(0)
        return f"{p.name} ({getattr(p, 'gcnArchName', '?').split(':')[0]}, {p.multi_processor_count} CUs)"
    except Exception as e:  # noqa: BLE001
        return f"unknown ({type(e).__name__})"


def table(recs):
    head = "field         log_n x batch order   |  copy/2   eval 1   eval 4 | intt+ev 1 intt+ev 4 | copy*1.5   divide  on domain | intt+div+ntt | b1/e1  b4/e4  bd/d"
    lines = [head]
    for r in recs:
        m = r["median_ms"]
        lines.append("%-13s %5d x %-5d %-7s | %7.3f  %7.3f  %7.3f | %9.3f %9.3f | %8.3f  %7.3f  %9.3f | %12.3f | %5.2f  %5.2f  %5.2f" % (
            FIELD[r["field"]], r["log_n"], r["batch"], ORDER[r["order"]], m["ce"], m["e1"], m["e4"], m["b1"], m["b4"], m["cd"], m["d"], m["o"], m["bd"],
            m["b1"] / m["e1"], m["b4"] / m["e4"], m["bd"] / m["d"]))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=DEFAULT_CONFIGS)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import field_ref as fr
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
            field, log_n, batch = (int(x) for x in spec.split(":"))
            fid, n = po.FR_OF[field], 1 << log_n
            nbytes = batch * n * 32
            r = fr.modulus(field)
            omega = po.root_of_unity(fid, log_n)
            w = fr.plain(field, omega)[0]
            pts = po.gen_scalars(fid, 0x1A6 + log_n, 4)
            on = fr.wire_one(field, pow(w, n // 2 + 5, r))
            op, pp, onp = C.c_void_p(omega.ctypes.data), C.c_void_p(pts.ctypes.data), C.c_void_p(on.ctypes.data)
            evals, quot, wa, wb = DeviceBuffer(nbytes), DeviceBuffer(nbytes), DeviceBuffer(nbytes), DeviceBuffer(nbytes)
            big_src, big_dst = DeviceBuffer(3 * nbytes // 2), DeviceBuffer(3 * nbytes // 2)
            vals, bvals, rems = np.zeros((batch, 4, 8), np.uint32), np.zeros((batch, 4, 8), np.uint32), np.zeros((batch, 8), np.uint32)
            vp, bvp, rp = C.c_void_p(vals.ctypes.data), C.c_void_p(bvals.ctypes.data), C.c_void_p(rems.ctypes.data)
            stream = gm.exec_stream.raw
            flag = C.c_uint(0)
            try:
                ffi.check(lib.panda_gen_scalars(field, 0x1A9 + log_n, 0, batch * n, evals.ptr, NULL_STREAM), "gen")
                ffi.check(lib.panda_stream_sync(NULL_STREAM), "sync")
                for order in (0, 1):
                    inverse, forward = (ffi.NTT_INVERSE, ffi.NTT_FORWARD) if order == 0 else (ffi.NTT_INVERSE_BITREV_IN, ffi.NTT_BITREV_OUT)

                    def transform(kind, src):
                        """one batched transform from src, the other of (wa, wb) as its second buffer -> the buffer that holds the result"""
                        other = wb if src is wa else wa
                        cfg = ffi.NttconfigurationV1(gm.mem_pool, stream, src.ptr, other.ptr, op, log_n, C.pointer(flag))
                        ffi.check(lib.panda_ntt_execute_batch(field, kind, cfg, batch, None), "ntt")
                        return other if flag.value else src

                    def route_b_eval(k):
                        ffi.check(lib.panda_poly_evaluate(field, transform(inverse, wa).ptr, n, batch, pp, k, bvp, stream), "evaluate")

                    def route_b_divide():
                        c = transform(inverse, wa)
                        ffi.check(lib.panda_poly_divide_linear(field, c.ptr, c.ptr, n, batch, pp, rp, stream), "divide")
                        return transform(forward, c)

                    def lag_eval(k):
                        ffi.check(lib.panda_poly_evaluate_lagrange(field, evals.ptr, log_n, batch, op, None, order, pp, k, vp, stream), "evaluate_lagrange")

                    def lag_divide(point):
                        ffi.check(lib.panda_poly_divide_linear_lagrange(field, evals.ptr, quot.ptr, log_n, batch, op, None, order, point, rp, stream), "divide_lagrange")

                    def refill():  # route (b) consumes its input
                        ffi.check(lib.panda_memcpy(wa.ptr, evals.ptr, nbytes), "copy")
                        ffi.check(lib.panda_stream_sync(NULL_STREAM), "sync")  # outside the timed call

                    def copy(count):  # a device-to-device panda_memcpy returns before the copy has run
                        ffi.check(lib.panda_memcpy(big_dst.ptr, big_src.ptr, count), "copy")
                        ffi.check(lib.panda_stream_sync(NULL_STREAM), "sync")

                    run = {"ce": lambda: copy(nbytes // 2), "cd": lambda: copy(3 * nbytes // 2),
                           "e1": lambda: lag_eval(1), "e4": lambda: lag_eval(4), "d": lambda: lag_divide(pp), "o": lambda: lag_divide(onp),
                           "b1": lambda: route_b_eval(1), "b4": lambda: route_b_eval(4), "bd": route_b_divide}
                    consumes = ("b1", "b4", "bd")
                    # the two routes agree before either is timed
                    lag_eval(4)
                    refill()
                    route_b_eval(4)
                    if not np.array_equal(vals, bvals):
                        raise SystemExit(f"field {field} 2^{log_n} x {batch} {ORDER[order]}: the values differ from the coefficient route's")
                    lag_divide(pp)
                    refill()
                    res = route_b_divide()
                    if not np.array_equal(quot.to_host(np.uint32), res.to_host(np.uint32)):
                        raise SystemExit(f"field {field} 2^{log_n} x {batch} {ORDER[order]}: the quotient differs from the coefficient route's")
                    ms = {arm: [] for arm in ARMS}
                    for rnd in range(a.rounds + 1):  # round 0 is the warm-up
                        for arm in ARMS:
                            if arm in consumes:
                                refill()
                            t0 = time.perf_counter()
                            run[arm]()
                            if rnd:
                                ms[arm].append((time.perf_counter() - t0) * 1e3)
                    med = {arm: statistics.median(ms[arm]) for arm in ARMS}
                    plan = [C.c_uint(0) for _ in range(4)]
                    ffi.check(lib.panda_poly_lagrange_plan(log_n, batch, 4, *[C.byref(x) for x in plan]), "plan")
                    rec = {"field": field, "log_n": log_n, "batch": batch, "order": order, "bytes": nbytes, "device": name, "tile": plan[0].value,
                           "launches_evaluate": plan[1].value, "launches_divide": plan[2].value, "rounds": a.rounds,
                           "per_call_ms": {arm: [round(v, 4) for v in ms[arm]] for arm in ARMS}, "median_ms": {arm: round(med[arm], 4) for arm in ARMS},
                           "eval1_gelem_per_s": round(batch * n / med["e1"] / 1e6, 3), "divide_gelem_per_s": round(batch * n / med["d"] / 1e6, 3)}
                    recs.append(rec)
                    line = json.dumps(rec)
                    print(line, flush=True)
                    if out:
                        out.write(line + "\n")
                        out.flush()
            finally:
                for d in (evals, quot, wa, wb, big_src, big_dst):
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
