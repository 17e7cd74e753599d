"""The measurement panda_field_batch_inverse / panda_poly_grand_product stand on.  There is no earlier way to do the step on the device, so
the yardstick is the stream floor: a device-to-device panda_memcpy of batch x n x 32 bytes (one read and one write of every byte; the
inverse reads its input twice and writes once, the product reads two inputs twice and writes once), as
  arm M: panda_memcpy, numerators -> the output buffer;
  arm V: panda_field_batch_inverse over the batch x n elements end to end, out of place;     arm v: in place;
  arm G: panda_poly_grand_product out of place;     arm g: in place on the numerators;     arm R: d_den == NULL (the running product);
  arm m: arm M again (the A/A of the baseline: its run-to-run spread in the same alternation).
A configuration of n = 1 is the latency split: the three launches and the one inversion with no data behind them.  One process, the arms
share their buffers.  Before anything is timed (up to --verify-max elements) the outputs are compared: in place against out of place
byte for byte, and both calls against their complete characterisations -- out_i in_i = one; out_0 = one, out_(i+1) den_i = out_i num_i,
totals den_(n-1) = out_(n-1) num_(n-1) -- by the CPU oracle's vector products.  Every shape is warmed up, wall clock around calls that end
in the library's own synchronise, the arms alternated --alternations times, each arm timed over enough calls to last --min-seconds.
Milliseconds per call.  One JSON line per configuration, then a table with the ratios to the copy.

usage: poly_product_bench.py [--configs field:n:batch,...] [--alternations N] [--min-seconds S] [--out FILE] [--verify-max ELEMS]"""
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

DEFAULT_CONFIGS = "0:1:1,0:65536:1,0:65536:8,0:1048576:1,0:1048576:8,0:16777216:1,0:16777216:8,0:1048579:1,0:1048579:8"
FIELD = ("BN254 Fr", "BLS12-377 Fr", "BLS12-381 Fr")
ARMS = "MVvGgRm"


def device_name():
    try:
        import torch
        p = torch.cuda.get_device_properties(0)
        return f"{p.name} ({getattr(p, 'gcnArchName', '?').split(':')[0]}, {p.multi_processor_count} CUs)"
    except Exception as e:  # noqa: BLE001
        return f"unknown ({type(e).__name__})"


def table(recs):
    lines = ["field         n x batch              MiB   | M copy (min / med / max ms)   | m med    spread  | inverse    x copy | in place   x copy | product    x copy | in place   x copy | no den     x copy | inverse G elem/s  product G elem/s"]
    for r in recs:
        med, ratio = r["median_ms"], r["ratio_to_copy"]
        lines.append("%-13s %-9d x %-3d %9.1f | %8.4f /%8.4f /%8.4f | %8.4f %7.4f | %9.4f %7.2f | %9.4f %7.2f | %9.4f %7.2f | %9.4f %7.2f | %9.4f %7.2f | %15.3f %17.3f" % (
            FIELD[r["field"]], r["n"], r["batch"], r["bytes"] / 2**20, *r["M_min_med_max"], med["m"], r["baseline_spread_ms"],
            med["V"], ratio["V"], med["v"], ratio["v"], med["G"], ratio["G"], med["g"], ratio["g"], med["R"], ratio["R"],
            r["inverse_gelem_per_s"], r["product_gelem_per_s"]))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=DEFAULT_CONFIGS)
    ap.add_argument("--alternations", type=int, default=10)
    ap.add_argument("--min-seconds", type=float, default=0.2)
    ap.add_argument("--out")
    ap.add_argument("--verify-max", type=int, default=1 << 24)
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
            elems = batch * n
            nbytes = elems * 32
            num, den, dst, work = (DeviceBuffer(nbytes) for _ in range(4))
            tot = np.zeros((batch, 8), np.uint32)
            tp = C.c_void_p(tot.ctypes.data)
            stream = gm.exec_stream.raw
            try:
                ffi.check(lib.panda_gen_scalars(field, 0x0CE + n, 0, elems, num.ptr, NULL_STREAM), "gen")
                ffi.check(lib.panda_gen_scalars(field, 0x1CE + n, 0, elems, den.ptr, NULL_STREAM), "gen")
                ffi.check(lib.panda_stream_sync(NULL_STREAM), "sync")
                ffi.check(lib.panda_memcpy(work.ptr, num.ptr, nbytes), "copy")

                def run_copy():  # a device-to-device copy returns before it has run: the call ends in a synchronise, like the library's
                    ffi.check(lib.panda_memcpy(dst.ptr, num.ptr, nbytes), "copy")
                    ffi.check(lib.panda_stream_sync(NULL_STREAM), "sync")

                def run_inverse(src, to):
                    ffi.check(lib.panda_field_batch_inverse(field, src.ptr, to.ptr, elems, stream), "inverse")

                def run_product(src, d, to):
                    ffi.check(lib.panda_poly_grand_product(field, src.ptr, d.ptr if d else None, to.ptr, n, batch, tp, stream), "product")

                # the in-place arms run on a buffer of their own: after the first call they work on earlier outputs, which cost the same
                run = {"M": run_copy, "V": lambda: run_inverse(num, dst), "v": lambda: run_inverse(work, work), "G": lambda: run_product(num, den, dst),
                       "g": lambda: run_product(work, den, work), "R": lambda: run_product(num, None, dst), "m": run_copy}
                verified = elems <= a.verify_max
                if verified:
                    one = po.f_vec(fid, po.OP_TO_MONT, np.array([[1, 0, 0, 0, 0, 0, 0, 0]], np.uint32))[0]
                    x = num.to_host(np.uint32).reshape(elems, 8)
                    d = den.to_host(np.uint32).reshape(elems, 8)
                    if not (np.any(x, axis=1).all() and np.any(d, axis=1).all()):
                        raise SystemExit(f"field {field} {n} x {batch}: the generated data holds a zero")
                    run["v"]()
                    in_place = work.to_host(np.uint32).reshape(elems, 8)
                    run["V"]()
                    inv = dst.to_host(np.uint32).reshape(elems, 8)
                    if not np.array_equal(inv, in_place):
                        raise SystemExit(f"field {field} {n} x {batch}: the inverse in place differs from out of place")
                    if not np.array_equal(po.f_vec(fid, po.OP_MUL, inv, x), np.broadcast_to(one, (elems, 8))):
                        raise SystemExit(f"field {field} {n} x {batch}: not the inverses")
                    ffi.check(lib.panda_memcpy(work.ptr, num.ptr, nbytes), "copy")
                    run["g"]()
                    in_place, tot_in_place = work.to_host(np.uint32).reshape(batch, n, 8), tot.copy()
                    run["G"]()
                    z = dst.to_host(np.uint32).reshape(batch, n, 8)
                    if not (np.array_equal(z, in_place) and np.array_equal(tot, tot_in_place)):
                        raise SystemExit(f"field {field} {n} x {batch}: the product in place differs from out of place")
                    x, d = x.reshape(batch, n, 8), d.reshape(batch, n, 8)
                    for p in range(batch):
                        step = po.f_vec(fid, po.OP_MUL, z[p], x[p])
                        nxt = np.concatenate([z[p, 1:], tot[p:p + 1]])
                        if not (np.array_equal(z[p, 0], one) and np.array_equal(po.f_vec(fid, po.OP_MUL, nxt, d[p]), step)):
                            raise SystemExit(f"field {field} {n} x {batch}: vector {p} is not the running product")
                    del x, d, z, inv, in_place
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
                ti, tpr, chunk, launches = C.c_uint(0), C.c_uint(0), C.c_uint(0), C.c_uint(0)
                ffi.check(lib.panda_poly_product_plan(n, batch, C.byref(ti), C.byref(tpr), C.byref(chunk), C.byref(launches)), "plan")
                rec = {"field": field, "n": n, "batch": batch, "bytes": nbytes, "device": name, "tile_inverse": ti.value, "tile_product": tpr.value,
                       "carry_chunk": chunk.value, "launches": launches.value, "verified": verified, "calls_per_repetition": reps,
                       "per_call_ms": {arm: [round(v, 5) for v in ms[arm]] for arm in ARMS},
                       "median_ms": {arm: round(med[arm], 5) for arm in ARMS},
                       "M_min_med_max": [round(min(ms["M"]), 5), round(med["M"], 5), round(max(ms["M"]), 5)],
                       "baseline_spread_ms": round(spread, 5),
                       "ratio_to_copy": {arm: round(med[arm] / med["M"], 4) for arm in "VvGgR"},
                       "copy_gb_per_s": round(2 * nbytes / med["M"] / 1e6, 1),
                       "inverse_gelem_per_s": round(elems / med["V"] / 1e6, 3),
                       "product_gelem_per_s": round(elems / med["G"] / 1e6, 3)}
                recs.append(rec)
                line = json.dumps(rec)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
            finally:
                for b in (num, den, dst, work):
                    b.free()
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
